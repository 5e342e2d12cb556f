// Single-linkage clustering on device without an N x N matrix: the minimum spanning tree of the distance graph by Boruvka rounds.
//
// Replaces hac.linkage(squareform(D), 'single') of get_facial_clusters (facial_clustering.py:243-245) and the O(N^2) host distance
// matrix of perform_clustering (process_photos.py:45-60).  The two distance sources (features on the fp32 MFMA, or a caller's fp64
// matrix read as its upper triangle) are linkage_scan.h's; they share every kernel but the first of a round.
// Edges are ordered strictly by (w, lower endpoint, higher endpoint); under that total order the lightest edge leaving every component
// is unique and the chosen edges close no cycle but mutual picks.  A round:
//   1. row_min_*      for every row i: the least (w, j) with j outside i's component (for a fixed row the total order is (w, j)); one
//                     workgroup owns its rows across the whole width, so no atomics;
//   2. comp_min1/2    per component: atomicMin of the orderable 64-bit key of w, then, among rows that hold that key, of (lo << 32 | hi);
//   3. hook           every root hooks under the root across its edge and appends the edge; of a mutual pair only the higher root does;
//   4. jump x J       pointer jumping on par[] until every vertex points at its root (J covers the depth bound of the round);
//   5. relabel        label = par.
// ceil(log2 n) rounds are launched with no host synchronisation (each round at least halves the components that still have a candidate
// edge); the device component count, and a flag raised by a round that hooked nothing, turn rounds after completion into early exits.
// dbscan.hip runs the same rounds with a candidate filter (both ends core, w <= eps): its core clusters are the components.
// Workspace: O(n), stream-ordered (hipMallocAsync), as hsefr_nn1's.
#include "linkage_scan.h"

namespace hsefr {

namespace {

using link::better;
using link::u64;

constexpr u64 NO_KEY = ~0ull;

// doubles -> unsigned keys in the same order (-0 folded into +0; NaN never reaches here: the callers reject non-finite input)
__device__ __forceinline__ u64 order_key(double v) {
    if (v == 0.0) v = 0.0;
    const u64 b = (u64)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ double key_value(u64 k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// cnt[0] components, cnt[1] hooks so far, cnt[2] hooks at the end of the previous round, cnt[3] "a round hooked nothing"
__device__ __forceinline__ bool rounds_done(const int* cnt) { return cnt[0] <= 1 || cnt[3] != 0; }

__global__ __launch_bounds__(256) void sl_init_kernel(int* __restrict__ label, int* __restrict__ cnt, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) label[i] = i;
    if (i == 0) { cnt[0] = n; cnt[1] = 0; cnt[2] = 0; cnt[3] = 0; }
}

__global__ __launch_bounds__(256) void sl_reset_kernel(const int* __restrict__ label, int* __restrict__ par, u64* __restrict__ cmin_w,
                                                       u64* __restrict__ cmin_e, const int* __restrict__ cnt, int n) {
    if (rounds_done(cnt)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    par[i] = label[i];
    cmin_w[i] = NO_KEY;
    cmin_e[i] = NO_KEY;
}

// FILTER: an edge is a candidate only if both ends are core and w <= eps; a workgroup whose rows are all non-core has none
template <bool FILTER>
__global__ __launch_bounds__(256) void sl_row_min_feat_kernel(const float* __restrict__ x, int n, int d, const float* __restrict__ born,
                                                              const float* __restrict__ year, const int* __restrict__ label,
                                                              const int* __restrict__ cnt, const unsigned char* __restrict__ core,
                                                              float eps, u64* __restrict__ row_key, int* __restrict__ row_j) {
    if (rounds_done(cnt)) return;
    __shared__ float s_val[4][32];
    __shared__ int s_idx[4][32];
    const int q0 = blockIdx.x * 32;
    if (FILTER && !__syncthreads_or(threadIdx.x < 32 && q0 + (int)threadIdx.x < n && core[q0 + threadIdx.x])) {
        if (threadIdx.x < 32 && q0 + (int)threadIdx.x < n) { row_key[q0 + threadIdx.x] = NO_KEY; row_j[q0 + threadIdx.x] = -1; }
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31;
    link::FeatScan fs(x, n, d, born, year);

    float best_v[16];
    int best_i[16], lab_r[16];
    bool core_r[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        lab_r[r] = label[fs.row(r)];
        core_r[r] = FILTER ? core[fs.row(r)] != 0 : true;
        best_v[r] = INFINITY;
        best_i[r] = 0x7fffffff;
    }

    const int tiles = (n + 31) / 32;
    for (int gt = wave; gt < tiles; gt += 4) {
        const int gcol = gt * 32 + li;
        const int grow = min(gcol, n - 1);
        const int glab = label[grow];
        const bool gcore = FILTER ? core[grow] != 0 : true;
        float v[16];
        fs.tile(grow, v);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const bool cand = !FILTER || (gcore && core_r[r] && v[r] <= eps);
            if (gcol < n && glab != lab_r[r] && cand && better(v[r], gcol, best_v[r], best_i[r])) { best_v[r] = v[r]; best_i[r] = gcol; }
        }
    }
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
            s_val[wave][fs.rr(r)] = best_v[r];
            s_idx[wave][fs.rr(r)] = best_i[r];
        }
    }
    __syncthreads();
    if (threadIdx.x < 32 && q0 + threadIdx.x < n) {
        float bv = s_val[0][threadIdx.x];
        int bi = s_idx[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (better(s_val[w][threadIdx.x], s_idx[w][threadIdx.x], bv, bi)) { bv = s_val[w][threadIdx.x]; bi = s_idx[w][threadIdx.x]; }
        const bool found = bi != 0x7fffffff;
        row_key[q0 + threadIdx.x] = found ? order_key((double)bv) : NO_KEY;
        row_j[q0 + threadIdx.x] = found ? bi : -1;
    }
}

template <bool FILTER>
__global__ __launch_bounds__(256) void sl_row_min_dense_kernel(const double* __restrict__ D, int n, const int* __restrict__ label,
                                                               const int* __restrict__ cnt, const unsigned char* __restrict__ core,
                                                               double eps, u64* __restrict__ row_key, int* __restrict__ row_j) {
    if (rounds_done(cnt)) return;
    __shared__ double s_t[64][65];
    __shared__ int s_lab[64];
    const int t = threadIdx.x, ri = t >> 2, sub = t & 3;
    const int r0 = blockIdx.x * 64, row = r0 + ri;
    if (FILTER && !__syncthreads_or(t < 64 && r0 + t < n && core[r0 + t])) {
        if (sub == 0 && row < n) { row_key[row] = NO_KEY; row_j[row] = -1; }
        return;
    }
    const int my_lab = row < n ? label[row] : -1;
    const bool my_core = FILTER ? row < n && core[row] != 0 : true;
    double bv = INFINITY;
    int bi = 0x7fffffff;
    for (int c0 = 0; c0 < n; c0 += 64) {
        __syncthreads();                                     // the previous tile has been read
        link::dense_stage(D, n, r0, c0, s_t);
        // a non-core column takes no label a core row can hold
        if (t < 64) s_lab[t] = c0 + t < n && (!FILTER || core[c0 + t]) ? label[c0 + t] : -1;
        __syncthreads();
#pragma unroll 4
        for (int m = 0; m < 16; ++m) {
            const int cj = sub + 4 * m, col = c0 + cj;
            const double v = link::dense_at(s_t, r0, c0, ri, cj);
            const bool cand = !FILTER || (my_core && s_lab[cj] >= 0 && v <= eps);
            if (col < n && s_lab[cj] != my_lab && cand && better(v, col, bv, bi)) { bv = v; bi = col; }
        }
    }
#pragma unroll
    for (int m = 1; m <= 2; m <<= 1) {
        const double ov = __shfl_xor(bv, m);
        const int oi = __shfl_xor(bi, m);
        if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (sub == 0 && row < n) {
        const bool found = bi != 0x7fffffff;
        row_key[row] = found ? order_key(bv) : NO_KEY;
        row_j[row] = found ? bi : -1;
    }
}

__global__ __launch_bounds__(256) void sl_comp_min1_kernel(const int* __restrict__ label, const u64* __restrict__ row_key,
                                                           u64* __restrict__ cmin_w, const int* __restrict__ cnt, int n) {
    if (rounds_done(cnt)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = row_key[i];
    if (k != NO_KEY) atomicMin(&cmin_w[label[i]], k);
}

__global__ __launch_bounds__(256) void sl_comp_min2_kernel(const int* __restrict__ label, const u64* __restrict__ row_key,
                                                           const int* __restrict__ row_j, const u64* __restrict__ cmin_w,
                                                           u64* __restrict__ cmin_e, const int* __restrict__ cnt, int n) {
    if (rounds_done(cnt)) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = row_key[i];
    const int c = label[i];
    if (k == NO_KEY || k != cmin_w[c]) return;
    const int j = row_j[i];
    const u64 lo = (u64)(i < j ? i : j), hi = (u64)(i < j ? j : i);
    atomicMin(&cmin_e[c], (lo << 32) | hi);
}

// Roots read label[] only and write par[] only, so no hook sees another's write.  cnt[0] may drop while this kernel runs; a root that reads
// it at <= 1 finds every hook of the round already counted, so it has none to make.  Edge slots and the component count take one atomic
// per wavefront (ballot + prefix count), not one per root.  edge_a == nullptr: the edges are not recorded.
__global__ __launch_bounds__(256) void sl_hook_kernel(const int* __restrict__ label, int* __restrict__ par, const u64* __restrict__ cmin_w,
                                                      const u64* __restrict__ cmin_e, int* __restrict__ cnt, int* __restrict__ edge_a,
                                                      int* __restrict__ edge_b, double* __restrict__ edge_h, int n) {
    if (*(volatile const int*)cnt <= 1 || cnt[3] != 0) return;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 256 + threadIdx.x;
    bool hook = false;
    int lo = 0, hi = 0, tgt = 0;
    if (r < n && label[r] == r) {
        const u64 e = cmin_e[r];
        if (e != NO_KEY) {
            lo = (int)(e >> 32);
            hi = (int)(e & 0xffffffffu);
            tgt = label[label[lo] == r ? hi : lo];
            hook = !(r < tgt && cmin_e[tgt] == e);     // mutual pick: the higher root hooks and records the edge
        }
    }
    const u64 m = __ballot(hook);
    if (m == 0) return;
    const int leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) {
        base = atomicAdd(&cnt[1], __popcll(m));
        atomicSub(&cnt[0], __popcll(m));
    }
    base = __shfl(base, leader);
    if (!hook) return;
    par[r] = tgt;
    const int slot = base + __popcll(m & ((1ull << lane) - 1));
    if (edge_a && slot < n - 1) {
        edge_a[slot] = lo;
        edge_b[slot] = hi;
        edge_h[slot] = key_value(cmin_w[r]);
    }
}

// in place: a concurrent update only moves par[p] closer to the root, so every pass still at least halves each distance to it
__global__ __launch_bounds__(256) void sl_jump_kernel(int* par, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int p = par[i], pp = par[p];
    if (pp != p) par[i] = pp;
}

// ends the round: a round that hooked nothing leaves nothing for the next ones (with a filter, components can stop while several remain)
__global__ __launch_bounds__(256) void sl_relabel_kernel(int* __restrict__ label, const int* __restrict__ par, int* __restrict__ cnt, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) label[i] = par[i];
    if (i == 0) {
        const int hooks = cnt[1];
        if (hooks == cnt[2]) cnt[3] = 1;
        else cnt[2] = hooks;
    }
}

int ceil_log2(long long v) {
    int k = 0;
    while ((1ll << k) < v) ++k;
    return k;
}

}  // namespace

// u64 arrays first: row_key, cmin_w, cmin_e; then int arrays: label, par, row_j, cnt[4]
size_t boruvka_bytes(int n) { return (size_t)n * 3 * 8 + (size_t)n * 3 * 4 + 16; }

int* boruvka_rounds(const DistSource& src, const unsigned char* core, float eps_f, double eps, char* ws, int* edge_a, int* edge_b,
                    double* edge_h, hipStream_t s) {
    const int n = src.n;
    u64* row_key = (u64*)ws;
    u64* cmin_w = row_key + n;
    u64* cmin_e = cmin_w + n;
    int* label = (int*)(cmin_e + n);
    int* par = label + n;
    int* row_j = par + n;
    int* cnt = row_j + n;
    const dim3 blk(256), g1((n + 255) / 256);
    HSEFR_LAUNCH(sl_init_kernel, g1, blk, 0, s, label, cnt, n);
    const int rounds = ceil_log2(n);
    for (int k = 0; k < rounds; ++k) {
        HSEFR_LAUNCH(sl_reset_kernel, g1, blk, 0, s, label, par, cmin_w, cmin_e, cnt, n);
        if (src.dense && core)
            HSEFR_LAUNCH(sl_row_min_dense_kernel<true>, dim3((n + 63) / 64), blk, 0, s, src.dense, n, label, cnt, core, eps, row_key, row_j);
        else if (src.dense)
            HSEFR_LAUNCH(sl_row_min_dense_kernel<false>, dim3((n + 63) / 64), blk, 0, s, src.dense, n, label, cnt, core, eps, row_key, row_j);
        else if (core)
            HSEFR_LAUNCH(sl_row_min_feat_kernel<true>, dim3((n + 31) / 32), blk, 0, s, src.x, n, src.d, src.born, src.year, label, cnt, core,
                         eps_f, row_key, row_j);
        else
            HSEFR_LAUNCH(sl_row_min_feat_kernel<false>, dim3((n + 31) / 32), blk, 0, s, src.x, n, src.d, src.born, src.year, label, cnt, core,
                         eps_f, row_key, row_j);
        HSEFR_LAUNCH(sl_comp_min1_kernel, g1, blk, 0, s, label, row_key, cmin_w, cnt, n);
        HSEFR_LAUNCH(sl_comp_min2_kernel, g1, blk, 0, s, label, row_key, row_j, cmin_w, cmin_e, cnt, n);
        HSEFR_LAUNCH(sl_hook_kernel, g1, blk, 0, s, label, par, cmin_w, cmin_e, cnt, edge_a, edge_b, edge_h, n);
        // round k starts with at most ceil(n / 2^k) components that can still hook: a hook tree over them is at most that deep, and a
        // vertex sits one step below its old root
        const long long comps = ((long long)n + (1ll << k) - 1) >> k;
        const int jumps = ceil_log2(comps + 1);
        for (int j = 0; j < jumps; ++j) HSEFR_LAUNCH(sl_jump_kernel, g1, blk, 0, s, par, n);
        HSEFR_LAUNCH(sl_relabel_kernel, g1, blk, 0, s, label, par, cnt, n);
    }
    return label;
}

int launch_single_linkage(const DistSource& src, int* edge_a, int* edge_b, double* edge_h, hipStream_t s) {
    const int n = src.n;
    if (n == 1) return HSEFR_OK;
    const size_t bytes = boruvka_bytes(n);
    char* ws = nullptr;
    if (hipMallocAsync((void**)&ws, bytes, s) != hipSuccess || !ws) {
        (void)hipGetLastError();
        set_error("single_linkage: no stream-ordered workspace (%zu bytes) for n=%d", bytes, n);
        return HSEFR_ERR_NOMEM;
    }
    boruvka_rounds(src, nullptr, 0.f, 0.0, ws, edge_a, edge_b, edge_h, s);
    const int rc = launch_status("single_linkage");
    (void)hipFreeAsync(ws, s);
    return rc;
}

}  // namespace hsefr
