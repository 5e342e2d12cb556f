// Single-linkage clustering on device without an N x N matrix: the minimum spanning tree of the distance graph by Boruvka rounds.
//
// Replaces hac.linkage(squareform(D), 'single') of get_facial_clusters (facial_clustering.py:243-245) and the O(N^2) host distance
// matrix of perform_clustering (process_photos.py:45-60).  Two distance sources share every kernel but the first of a round:
//   features  w(i,j) = max(sqrt(max(|x_i|^2 + |x_j|^2 - 2 x_i.x_j, 0)) + 0.1 (born_j - born_i)^2 / (2 max(year_i, year_j) - born_i - born_j), 0)
//             (the age term only with born / year), the contraction on the fp32 MFMA as in nn1_kernel -- every w(i,j) is computed by the
//             same commutative expression from the same row norms and the same FMA chain whichever side of a tile i falls on, so the graph
//             is bitwise symmetric;
//   dense     a caller's fp64 D [n,n], read as its upper triangle D[min(i,j), max(i,j)] (what squareform(D, checks=False) reads).
// Edges are ordered strictly by (w, lower endpoint, higher endpoint); under that total order the lightest edge leaving every component
// is unique and the chosen edges close no cycle but mutual picks.  A round:
//   1. row_min_*      for every row i: the least (w, j) with j outside i's component (for a fixed row the total order is (w, j)); one
//                     workgroup owns its rows across the whole width, so no atomics;
//   2. comp_min1/2    per component: atomicMin of the orderable 64-bit key of w, then, among rows that hold that key, of (lo << 32 | hi);
//   3. hook           every root hooks under the root across its edge and appends the edge; of a mutual pair only the higher root does;
//   4. jump x J       pointer jumping on par[] until every vertex points at its root (J covers the depth bound of the round);
//   5. relabel        label = par.
// ceil(log2 n) rounds are launched with no host synchronisation (each round at least halves the components); the device component count
// turns rounds after completion into early exits.  Workspace: O(n), stream-ordered (hipMallocAsync), as hsefr_nn1's.
#include "common.h"

namespace hsefr {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned long long u64;

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

template <typename T>
__device__ __forceinline__ bool better(T v, int i, T bv, int bi) { return v < bv || (v == bv && i < bi); }

__global__ __launch_bounds__(256) void sl_init_kernel(int* __restrict__ label, int* __restrict__ cnt, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) label[i] = i;
    if (i == 0) { cnt[0] = n; cnt[1] = 0; }
}

__global__ __launch_bounds__(256) void sl_reset_kernel(const int* __restrict__ label, int* __restrict__ par, u64* __restrict__ cmin_w,
                                                       u64* __restrict__ cmin_e, const int* __restrict__ cnt, int n) {
    if (cnt[0] <= 1) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    par[i] = label[i];
    cmin_w[i] = NO_KEY;
    cmin_e[i] = NO_KEY;
}

// Features: one workgroup = 32 rows x all n columns, its 4 waves take column tiles of 32 round-robin (nn1_kernel's layout).  Row norms come
// from the fragments that feed the MFMAs: lane (li, half) sums the same elements in the same order for a row on either operand, and the
// halves meet in a commutative add, so |x_i|^2 is one value whichever side i is on.
__global__ __launch_bounds__(256) void sl_row_min_feat_kernel(const float* __restrict__ x, int n, int d, const float* __restrict__ born,
                                                              const float* __restrict__ year, const int* __restrict__ label,
                                                              const int* __restrict__ cnt, u64* __restrict__ row_key,
                                                              int* __restrict__ row_j) {
    if (cnt[0] <= 1) return;
    __shared__ float s_val[4][32];
    __shared__ int s_idx[4][32];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int q0 = blockIdx.x * 32;
    const float* qp = x + (size_t)min(q0 + li, n - 1) * d + 4 * lh;
    const bool age = born != nullptr;

    float best_v[16], born_r[16], year_r[16];
    int best_i[16], lab_r[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = min(q0 + (r & 3) + 8 * (r >> 2) + 4 * lh, n - 1);
        lab_r[r] = label[row];
        born_r[r] = age ? born[row] : 0.f;
        year_r[r] = age ? year[row] : 0.f;
        best_v[r] = INFINITY;
        best_i[r] = 0x7fffffff;
    }

    float qq = 0.f;  // |x_row|^2 (lane rr holds row q0 + rr), from the wave's first tile
    bool qq_done = false;
    const int tiles = (n + 31) / 32;
    for (int gt = wave; gt < tiles; gt += 4) {
        const int gcol = gt * 32 + li;
        const int grow = min(gcol, n - 1);
        const float* gp = x + (size_t)grow * d + 4 * lh;
        const int glab = label[grow];
        const float gb = age ? born[grow] : 0.f, gy = age ? year[grow] : 0.f;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        float gg = 0.f, qs = 0.f;
        for (int k = 0; k < d; k += 8) {
            const f32x4 a = *(const f32x4*)(qp + k);
            const f32x4 b = *(const f32x4*)(gp + k);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], b[j], acc, 0, 0, 0);
                gg = fmaf(b[j], b[j], gg);
                qs = fmaf(a[j], a[j], qs);
            }
        }
        gg += __shfl_xor(gg, 32);
        if (!qq_done) { qq = qs + __shfl_xor(qs, 32); qq_done = true; }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = (r & 3) + 8 * (r >> 2) + 4 * lh;
            const float s = __shfl(qq, rr) + gg;
            float v = sqrtf(fmaxf(fmaf(-2.f, acc[r], s), 0.f));
            if (age) {
                const float t = gb - born_r[r];
                const float den = 2.f * fmaxf(year_r[r], gy) - (born_r[r] + gb);
                v = fmaxf(v + 0.1f * (t * t) / den, 0.f);
            }
            if (gcol < n && glab != lab_r[r] && better(v, gcol, best_v[r], best_i[r])) { best_v[r] = v; best_i[r] = gcol; }
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
            const int rr = (r & 3) + 8 * (r >> 2) + 4 * lh;
            s_val[wave][rr] = best_v[r];
            s_idx[wave][rr] = best_i[r];
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

// Dense fp64: one workgroup = 64 rows x all n columns, walked in 64 x 64 tiles of the UPPER triangle staged through LDS with coalesced
// row reads -- tile (R, C) with C > R is read as it is, C < R from its mirror D[C, R] and transposed, C == R by (min, max).  Thread t
// holds row t / 4 and the columns t % 4 + 4 m of each tile.  Bandwidth-bound: every upper element is read twice per round.
__global__ __launch_bounds__(256) void sl_row_min_dense_kernel(const double* __restrict__ D, int n, const int* __restrict__ label,
                                                               const int* __restrict__ cnt, u64* __restrict__ row_key,
                                                               int* __restrict__ row_j) {
    if (cnt[0] <= 1) return;
    __shared__ double s_t[64][65];
    __shared__ int s_lab[64];
    const int t = threadIdx.x, ri = t >> 2, sub = t & 3;
    const int r0 = blockIdx.x * 64, row = r0 + ri;
    const int my_lab = row < n ? label[row] : -1;
    double bv = INFINITY;
    int bi = 0x7fffffff;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int sr0 = c0 < r0 ? c0 : r0, sc0 = c0 < r0 ? r0 : c0;
        __syncthreads();                                     // the previous tile has been read
#pragma unroll 4
        for (int k = 0; k < 16; ++k) {
            const int a = (t >> 6) + 4 * k, b = t & 63;
            const int gr = sr0 + a, gc = sc0 + b;
            s_t[a][b] = (gr < n && gc < n) ? D[(size_t)gr * n + gc] : 0.0;
        }
        if (t < 64) s_lab[t] = c0 + t < n ? label[c0 + t] : -1;
        __syncthreads();
#pragma unroll 4
        for (int m = 0; m < 16; ++m) {
            const int cj = sub + 4 * m, col = c0 + cj;
            const bool up = c0 > r0 || (c0 == r0 && ri < cj);
            const double v = up ? s_t[ri][cj] : s_t[cj][ri];
            if (col < n && s_lab[cj] != my_lab && better(v, col, bv, bi)) { bv = v; bi = col; }
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
    if (cnt[0] <= 1) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const u64 k = row_key[i];
    if (k != NO_KEY) atomicMin(&cmin_w[label[i]], k);
}

__global__ __launch_bounds__(256) void sl_comp_min2_kernel(const int* __restrict__ label, const u64* __restrict__ row_key,
                                                           const int* __restrict__ row_j, const u64* __restrict__ cmin_w,
                                                           u64* __restrict__ cmin_e, const int* __restrict__ cnt, int n) {
    if (cnt[0] <= 1) return;
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
// per wavefront (ballot + prefix count), not one per root.
__global__ __launch_bounds__(256) void sl_hook_kernel(const int* __restrict__ label, int* __restrict__ par, const u64* __restrict__ cmin_w,
                                                      const u64* __restrict__ cmin_e, int* __restrict__ cnt, int* __restrict__ edge_a,
                                                      int* __restrict__ edge_b, double* __restrict__ edge_h, int n) {
    if (*(volatile const int*)cnt <= 1) return;
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
    if (slot < n - 1) {
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

__global__ __launch_bounds__(256) void sl_relabel_kernel(int* __restrict__ label, const int* __restrict__ par, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) label[i] = par[i];
}

int ceil_log2(long long v) {
    int k = 0;
    while ((1ll << k) < v) ++k;
    return k;
}

}  // namespace

int launch_single_linkage(const float* x, int n, int d, const float* born, const float* year, const double* dense, int* edge_a, int* edge_b,
                          double* edge_h, hipStream_t s) {
    if (n == 1) return HSEFR_OK;
    // u64 arrays first: row_key, cmin_w, cmin_e; then int arrays: label, par, row_j, cnt[2]
    const size_t bytes = (size_t)n * 3 * 8 + (size_t)n * 3 * 4 + 16;
    char* ws = nullptr;
    if (hipMallocAsync((void**)&ws, bytes, s) != hipSuccess || !ws) {
        (void)hipGetLastError();
        set_error("single_linkage: no stream-ordered workspace (%zu bytes) for n=%d", bytes, n);
        return HSEFR_ERR_NOMEM;
    }
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
        if (dense)
            HSEFR_LAUNCH(sl_row_min_dense_kernel, dim3((n + 63) / 64), blk, 0, s, dense, n, label, cnt, row_key, row_j);
        else
            HSEFR_LAUNCH(sl_row_min_feat_kernel, dim3((n + 31) / 32), blk, 0, s, x, n, d, born, year, label, cnt, row_key, row_j);
        HSEFR_LAUNCH(sl_comp_min1_kernel, g1, blk, 0, s, label, row_key, cmin_w, cnt, n);
        HSEFR_LAUNCH(sl_comp_min2_kernel, g1, blk, 0, s, label, row_key, row_j, cmin_w, cmin_e, cnt, n);
        HSEFR_LAUNCH(sl_hook_kernel, g1, blk, 0, s, label, par, cmin_w, cmin_e, cnt, edge_a, edge_b, edge_h, n);
        // round k starts with at most ceil(n / 2^k) components: a hook tree over them is at most that deep, and a vertex sits one step below
        // its old root
        const long long comps = ((long long)n + (1ll << k) - 1) >> k;
        const int jumps = ceil_log2(comps + 1);
        for (int j = 0; j < jumps; ++j) HSEFR_LAUNCH(sl_jump_kernel, g1, blk, 0, s, par, n);
        HSEFR_LAUNCH(sl_relabel_kernel, g1, blk, 0, s, label, par, n);
    }
    const int rc = launch_status("single_linkage");
    (void)hipFreeAsync(ws, s);
    return rc;
}

}  // namespace hsefr
