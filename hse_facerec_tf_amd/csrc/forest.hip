// libhsefr_forest.so (include/hsefr_forest.h): a random forest fitted level by level and applied on the device.  The forest's
// definition -- hash, bootstrap, visiting order, candidates, score, threshold, leaves -- stands in the header and, word for word, in
// tests/random_forest_ref.py; this file equals that restatement bit for bit.
//
// The hash, once for the kernels: mix(z) is splitmix64's finaliser, and
//   hash(seed, tree, purpose, node, counter): h = mix(seed + G); for v in (tree, purpose, node, counter): h = mix(h + v + G)
// (forest_hash below).
//
// Fit.  A tree's distinct rows are a list of row indices, partitioned so that every node is a contiguous segment; a node's children
// are allocated level by level, so the nodes of one level of one tree are consecutive node indices [level_begin[L], level_begin[L+1])
// and the host never has to read anything back between levels: per level it launches, over the worst-case grid of that level,
//   order_kernel      (tree, node)           the node's first max_features features by the visiting key, a bitonic sort in LDS
//   search_kernel     (tree, node, feature)  the hot path: gather the feature's values over the node's rows, sort (value, row) keys --
//                                            in LDS for up to TILE rows, in a slab of global memory beyond (the same network, run by
//                                            the same workgroup) --, then scan the sorted segment once with the node's class counts
//                                            in LDS: moving weight w of class c from right to left changes S_L by 2 w L_c + w^2 and
//                                            S_R by -2 w R_c + w^2, so a step is O(1) whatever the class count; each candidate's
//                                            score is two fp64 divisions and one addition (-ffp-contract=off: nothing fuses)
//   choose_kernel     (tree, node)           the winner over the node's features (ties: the earlier feature, then the lower position);
//                                            without a candidate the visit goes on past max_features, feature by feature; a node
//                                            that stays unsplit becomes a leaf and its (class, count) list is written
//   partition_kernel  (tree, node)           children indices from the count of split nodes before this one, and one stable pass that
//                                            splits the node's rows into the other row buffer
// and after the last level choose_kernel once more, which turns every node at max_depth into a leaf.  Counts are integers and the
// only atomics are integer adds (bootstrap multiplicities in global memory, class counts in LDS), so the result has no order in it:
// two fits give the same bytes.  Every index derived from data (a label, a child, a leaf slot, a partition target) is checked against
// its bound before it is used; a violation sets HSEFR_FOREST_INFO_INTERNAL in d_info instead of writing.
//
// Predict.  One workgroup per probe; its probabilities are one fp64 vector in LDS, to which the trees' leaves are added in tree order.
//
// Shared with the other three libraries: nothing (linked with -fvisibility=hidden; this library has its own error string).
#include <hip/hip_runtime.h>

#include "../../include/hsefr_forest.h"
#include "lib_error.h"

using hsefr::g_error;
using hsefr::set_error;

#define FOREST_REQUIRE HSEFR_LIB_REQUIRE

namespace {

typedef unsigned long long u64;

// gfx950 store-data hazard: two wait states behind a wide store (tools/isa_lint.py); nothing on the host pass
#if defined(__HIP_DEVICE_COMPILE__)
#define STORE_DATA_GUARD() asm volatile("s_nop 1" ::: "memory")
#else
#define STORE_DATA_GUARD() \
    do {                   \
    } while (0)
#endif

constexpr int THREADS = 256;
constexpr int TILE = 4096;                              // rows of a node that are sorted in LDS; more go through the global slab
constexpr int MAX_CLASSES = HSEFR_FOREST_MAX_CLASSES;
constexpr int MAX_D = HSEFR_FOREST_MAX_D;
constexpr int CLASS_SHIFT = 20;                         // a sorted key's low word after the sort: class << 20 | weight (weight <= n < 2^16)
constexpr u64 GOLDEN = 0x9E3779B97F4A7C15ull;
constexpr u64 PURPOSE_BOOTSTRAP = 1, PURPOSE_FEATURE = 2;

__host__ __device__ inline u64 mix(u64 z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__host__ __device__ inline u64 forest_hash(u64 seed, u64 tree, u64 purpose, u64 node, u64 counter) {
    u64 h = mix(seed + GOLDEN);
    h = mix(h + tree + GOLDEN);
    h = mix(h + purpose + GOLDEN);
    h = mix(h + node + GOLDEN);
    return mix(h + counter + GOLDEN);
}

// float bits <-> a uint32 that orders as the floats do
__device__ __forceinline__ unsigned ordered(unsigned bits) { return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ float unordered(unsigned key) { return __uint_as_float(key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu)); }

__host__ __device__ inline int pow2_ceil(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// a candidate's score and threshold: one 16-byte store
struct __attribute__((aligned(16))) CandPair {
    double score, thr;
};

// the workspace of a fit, carved from d_workspace by layout()
struct Work {
    int* mult;          // [T, n]     bootstrap multiplicity of every row
    int* rows;          // [2, T, n]  a tree's distinct rows, partitioned; levels alternate between the two buffers
    int* level_begin;   // [T, D + 2] node index at which a level starts
    int* node_start;    // [T, M]     a node's segment of the tree's rows
    int* node_len;      // [T, M]
    unsigned* node_heap;  // [T, M]   heap number (root 1)
    int* split_pos;     // [T, M]     rows going left
    int* order;         // [T, W, mf] features a level's nodes visit first
    CandPair* cand;     // [T, W, mf] best candidate of (node, feature)
    int* cand_pos;      //            0: none; -1: the node holds one class (every feature's workgroup finds that)
    u64* slab;          // [T, mf, 2 n] sort space of segments above TILE (n > TILE only)
};

struct Sizes {
    int n, d, n_classes, T, D, mf, M, W;
    u64 seed;
};

size_t layout(const Sizes& z, char* base, Work* w) {
    size_t at = 0;
    auto take = [&](size_t bytes) {
        char* p = base ? base + at : nullptr;
        at += (bytes + 255) & ~(size_t)255;
        return p;
    };
    const size_t tn = (size_t)z.T * z.n, tm = (size_t)z.T * z.M, cands = (size_t)z.T * z.W * z.mf;
    Work local;
    Work& o = w ? *w : local;
    o.mult = (int*)take(tn * 4);
    o.rows = (int*)take(2 * tn * 4);
    o.level_begin = (int*)take((size_t)z.T * (z.D + 2) * 4);
    o.node_start = (int*)take(tm * 4);
    o.node_len = (int*)take(tm * 4);
    o.node_heap = (unsigned*)take(tm * 4);
    o.split_pos = (int*)take(tm * 4);
    o.order = (int*)take(cands * 4);
    o.cand = (CandPair*)take(cands * 16);
    o.cand_pos = (int*)take(cands * 4);
    o.slab = (u64*)take(z.n > TILE ? (size_t)z.T * z.mf * 2 * z.n * 8 : 0);
    return at;
}

// ---- workgroup helpers (THREADS threads, all of them call) ------------------------------------------------------------------------
__device__ u64 block_sum(u64 v, u64* buf) {
    const int tid = threadIdx.x;
    buf[tid] = v;
    __syncthreads();
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) buf[tid] += buf[tid + s];
        __syncthreads();
    }
    const u64 r = buf[0];
    __syncthreads();
    return r;
}

// exclusive prefix sum of v over the workgroup; *total: the sum
__device__ int block_scan(int v, u64* buf, int* total) {
    const int tid = threadIdx.x;
    buf[tid] = (u64)v;
    __syncthreads();
    for (int off = 1; off < THREADS; off <<= 1) {
        const u64 t = tid >= off ? buf[tid - off] : 0;
        __syncthreads();
        buf[tid] += t;
        __syncthreads();
    }
    const int incl = (int)buf[tid];
    *total = (int)buf[THREADS - 1];
    __syncthreads();
    return incl - v;
}

// ascending bitonic sort of a[0 .. P), P a power of two, by the workgroup; a is LDS or global memory
__device__ __forceinline__ void bitonic_sort(u64* a, int P) {
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P; i += THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const u64 x = a[i], y = a[l];
                    if ((x > y) == ((i & k) == 0)) {
                        a[i] = y;
                        a[l] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
}

struct SearchShared {
    u64 keys[TILE];             // 32 KB: the sort tile
    int left[MAX_CLASSES];      //  8 KB: class counts left of the scan
    int right[MAX_CLASSES];     //  8 KB: and right of it
    u64 red[THREADS];           //  2 KB: block_sum / block_scan
    double best_score, best_thr;
    int best_pos, pure;
};

struct Tree {
    const float* x;
    const int* labels;
    const int* mult;    // this tree's
    const int* rows;    // this tree's, the level's buffer
    int d, n_classes, n;
    int* info;
};

// a row of the tree's list, checked against n before anything is indexed with it
__device__ __forceinline__ int checked_row(const Tree& t, int at) {
    const int row = t.rows[at];
    if ((unsigned)row < (unsigned)t.n) return row;
    atomicOr(t.info, HSEFR_FOREST_INFO_INTERNAL);
    return 0;
}

struct Cand {
    double score, thr;
    int pos;            // 0: no candidate
    int pure;           // the node holds one class (then pos = 0)
};

// The best candidate of feature f over the node's segment [s, s + m) (m >= 2); `slab`: 2 n keys of global memory owned by this
// workgroup's (tree, feature slot), of which a node uses [2 s, 2 s + pow2_ceil(m)) -- disjoint between the nodes of a tree because
// their segments are and pow2_ceil(m) < 2 m.
// TILED: m <= TILE and the keys are sorted in LDS; otherwise in the slab.  Two instances, so that every access has its address space
// at compile time (one pointer that is LDS or global by a run-time choice would be a generic pointer).
template <bool TILED>
__device__ Cand scan_feature(SearchShared& sh, const Tree& t, int s, int m, int f, u64* slab) {
    const int tid = threadIdx.x;
    const int P = pow2_ceil(m);
    constexpr bool tiled = TILED;
    u64* a = TILED ? sh.keys : slab + 2 * (size_t)s;
    // keys (value, position in the segment); the node's classes' counters cleared
    for (int i = tid; i < P; i += THREADS) {
        u64 key = ~0ull;
        if (i < m) {
            const int row = checked_row(t, s + i);
            key = ((u64)ordered(__float_as_uint(t.x[(size_t)row * t.d + f])) << 32) | (unsigned)i;
            const int c = t.labels[row];
            if ((unsigned)c < (unsigned)t.n_classes) sh.left[c] = 0, sh.right[c] = 0;
        }
        a[i] = key;
    }
    __syncthreads();
    u64 n_part = 0;
    for (int i = tid; i < m; i += THREADS) {
        const int row = checked_row(t, s + i), c = t.labels[row], w = t.mult[row];
        if ((unsigned)c < (unsigned)t.n_classes) atomicAdd(&sh.right[c], w);      // integer: no order in the result
        n_part += (u64)w;
    }
    __syncthreads();
    u64 s_part = 0;                                                                // sum_c R_c^2 = sum_rows w R_class(row)
    for (int i = tid; i < m; i += THREADS) {
        const int row = checked_row(t, s + i), c = t.labels[row];
        if ((unsigned)c < (unsigned)t.n_classes) s_part += (u64)t.mult[row] * (u64)sh.right[c];
    }
    const u64 N = block_sum(n_part, sh.red), S = block_sum(s_part, sh.red);
    Cand out;
    out.score = 0.0, out.thr = 0.0, out.pos = 0, out.pure = S == N * N;
    if (out.pure) return out;                                                      // the same in every thread
    bitonic_sort(a, P);
    // a sorted key's low word becomes (class, weight): the scan then reads nothing but the keys and the counters
    for (int i = tid; i < m; i += THREADS) {
        const u64 key = a[i];
        const unsigned at = (unsigned)key;
        unsigned cw = 0;
        if (at < (unsigned)m) {
            const int row = checked_row(t, s + (int)at), c = t.labels[row];
            cw = ((unsigned)c < (unsigned)t.n_classes ? (unsigned)c << CLASS_SHIFT : 0u) | ((unsigned)t.mult[row] & ((1u << CLASS_SHIFT) - 1));
        }
        a[i] = (key & 0xffffffff00000000ull) | cw;
    }
    __syncthreads();
    // the scan: one thread walks the sorted segment, tile by tile; a tile of the slab is staged in LDS by all
    u64 S_L = 0, S_R = S, N_L = 0;
    double best = 0.0, lo = 0.0, hi = 0.0;
    int best_pos = 0;
    float prev = 0.f;
    for (int base = 0; base < m; base += TILE) {
        const int count = min(TILE, m - base);
        if (!tiled) {
            __syncthreads();
            for (int i = tid; i < count; i += THREADS) sh.keys[i] = a[base + i];
            __syncthreads();
        }
        if (tid == 0) {
            for (int i = 0; i < count; ++i) {
                const u64 key = sh.keys[i];
                const float cur = unordered((unsigned)(key >> 32));
                const int p = base + i;
                if (p > 0 && cur > prev) {                                          // a candidate: rows 0 .. p-1 left, p .. m-1 right
                    const double score = (double)S_L / (double)N_L + (double)S_R / (double)(N - N_L);
                    if (best_pos == 0 || score > best) best = score, best_pos = p, lo = (double)prev, hi = (double)cur;
                }
                const unsigned cw = (unsigned)key;
                const u64 w = cw & ((1u << CLASS_SHIFT) - 1);
                const int c = (int)(cw >> CLASS_SHIFT);                             // below MAX_CLASSES by construction
                const u64 l = (u64)sh.left[c], r = (u64)sh.right[c];
                S_L += 2 * w * l + w * w;
                S_R = S_R - 2 * w * r + w * w;
                sh.left[c] = (int)(l + w);
                sh.right[c] = (int)(r - w);
                N_L += w;
                prev = cur;
            }
        }
    }
    if (tid == 0) {
        double thr = lo / 2.0 + hi / 2.0;
        if (thr == hi || !isfinite(thr)) thr = lo;
        sh.best_score = best, sh.best_thr = thr, sh.best_pos = best_pos;
    }
    __syncthreads();
    out.score = sh.best_score, out.thr = sh.best_thr, out.pos = sh.best_pos;
    __syncthreads();
    return out;
}

// the node of (tree, j) at `level`, or -1 where the level has fewer nodes
__device__ __forceinline__ int level_node(const Work& w, const Sizes& z, int tree, int level, int j) {
    const int* lb = w.level_begin + (size_t)tree * (z.D + 2);
    const int begin = lb[level], end = lb[level + 1];
    return j < end - begin && begin + j < z.M ? begin + j : -1;
}

// the node's features by visiting key into keys[0 .. pow2_ceil(d)): the low 12 bits of a sorted key are the feature
__device__ void visiting_order(u64* keys, const Sizes& z, int tree, unsigned heap) {
    const int P = pow2_ceil(z.d);
    for (int i = threadIdx.x; i < P; i += THREADS)
        keys[i] = i < z.d ? ((forest_hash(z.seed, (u64)tree, PURPOSE_FEATURE, (u64)heap, (u64)i) >> 12 << 12) | (u64)i) : ~0ull;
    bitonic_sort(keys, P);
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------------
// one workgroup per tree: multiplicities, the distinct rows in ascending order, the root
__global__ __launch_bounds__(THREADS) void init_kernel(Work w, Sizes z, int bootstrap, int* n_nodes) {
    __shared__ u64 red[THREADS];
    const int tree = blockIdx.x, tid = threadIdx.x;
    int* mult = w.mult + (size_t)tree * z.n;
    for (int j = tid; j < z.n; j += THREADS) {
        if (bootstrap) {
            const u64 u = forest_hash(z.seed, (u64)tree, PURPOSE_BOOTSTRAP, 0, (u64)j) >> 32;
            const int row = (int)((u * (u64)z.n) >> 32);                            // < n
            atomicAdd(&mult[row], 1);
        } else {
            mult[j] = 1;
        }
    }
    __threadfence();
    __syncthreads();
    int* rows = w.rows + (size_t)tree * z.n;
    int base = 0;
    for (int i0 = 0; i0 < z.n; i0 += THREADS) {
        const int i = i0 + tid;
        // read where the atomics landed (a neighbour tree's workgroup on this CU may have cached the line before they did)
        const int flag = i < z.n && __hip_atomic_load(&mult[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0;
        int total;
        const int rank = block_scan(flag, red, &total);
        if (flag) rows[base + rank] = i;                                            // base + rank <= i < n
        base += total;
    }
    if (tid == 0) {
        const size_t node = (size_t)tree * z.M;
        w.node_start[node] = 0, w.node_len[node] = base, w.node_heap[node] = 1u;
        int* lb = w.level_begin + (size_t)tree * (z.D + 2);
        lb[0] = 0;
        for (int l = 1; l < z.D + 2; ++l) lb[l] = 1;
        n_nodes[tree] = 1;
    }
}

// the input's part of d_info: a label out of range, a value that is not finite
__global__ __launch_bounds__(THREADS) void validate_kernel(const float* x, const int* labels, Sizes z, int* info) {
    const size_t total = (size_t)z.n * z.d, stride = (size_t)gridDim.x * THREADS;
    int bits = 0;
    for (size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x; i < total; i += stride)
        if ((__float_as_uint(x[i]) & 0x7f800000u) == 0x7f800000u) bits |= HSEFR_FOREST_INFO_NOT_FINITE;
    for (size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x; i < (size_t)z.n; i += stride)
        if ((unsigned)labels[i] >= (unsigned)z.n_classes) bits |= HSEFR_FOREST_INFO_BAD_LABEL;
    if (bits) atomicOr(info, bits);
}

__global__ __launch_bounds__(THREADS) void order_kernel(Work w, Sizes z, int level) {
    __shared__ u64 keys[MAX_D];
    const int tree = blockIdx.y, j = blockIdx.x;
    const int node = level_node(w, z, tree, level, j);
    if (node < 0) return;
    const size_t at = (size_t)tree * z.M + node;
    if (w.node_len[at] < 2) return;
    visiting_order(keys, z, tree, w.node_heap[at]);
    int* order = w.order + ((size_t)tree * z.W + j) * z.mf;
    for (int k = threadIdx.x; k < z.mf; k += THREADS) order[k] = (int)(keys[k] & 4095u);
}

__global__ __launch_bounds__(THREADS) void search_kernel(Work w, Sizes z, const float* x, const int* labels, int level, int* info) {
    __shared__ SearchShared sh;
    const int tree = blockIdx.y, j = blockIdx.x, k = blockIdx.z;
    const int node = level_node(w, z, tree, level, j);
    if (node < 0) return;
    const size_t at = (size_t)tree * z.M + node, slot = ((size_t)tree * z.W + j) * z.mf + k;
    const int s = w.node_start[at], m = w.node_len[at];
    Cand c;
    c.score = 0.0, c.thr = 0.0, c.pos = 0, c.pure = 0;
    const int f = m >= 2 ? w.order[slot] : -1;
    if (m >= 2 && (unsigned)f < (unsigned)z.d && s >= 0 && s + m <= z.n) {
        Tree t = {x, labels, w.mult + (size_t)tree * z.n, w.rows + ((size_t)(level & 1) * z.T + tree) * z.n, z.d, z.n_classes, z.n, info};
        u64* slab = w.slab + ((size_t)tree * z.mf + k) * 2 * z.n;
        c = m <= TILE ? scan_feature<true>(sh, t, s, m, f, slab) : scan_feature<false>(sh, t, s, m, f, slab);
    }
    if (threadIdx.x == 0) {
        CandPair pair;
        pair.score = c.score, pair.thr = c.thr;
        w.cand[slot] = pair;
        STORE_DATA_GUARD();
        w.cand_pos[slot] = c.pure ? -1 : c.pos;
    }
}

// The leaf list of the segment [s, s + m): its classes sorted (TILED: in LDS, otherwise in the slab), one (class, count) pair per
// distinct class from slot s of the tree's list.  Returns the number of pairs.
template <bool TILED>
__device__ int write_leaf(SearchShared& q, const Tree& t, int s, int m, u64* slab, int* leaf_class, int* leaf_count) {
    const int tid = threadIdx.x;
    const int P = pow2_ceil(m);
    u64* a = TILED ? q.keys : slab + 2 * (size_t)s;
    for (int i = tid; i < P; i += THREADS) {
        u64 key = ~0ull;
        if (i < m) {
            const int c = t.labels[checked_row(t, s + i)];
            if ((unsigned)c < (unsigned)t.n_classes) key = (u64)c, q.right[c] = 0;
        }
        a[i] = key;
    }
    __syncthreads();
    for (int i = tid; i < m; i += THREADS) {
        const int row = checked_row(t, s + i), c = t.labels[row];
        if ((unsigned)c < (unsigned)t.n_classes) atomicAdd(&q.right[c], t.mult[row]);
    }
    bitonic_sort(a, P);
    int base = 0;
    for (int i0 = 0; i0 < m; i0 += THREADS) {
        const int i = i0 + tid;
        const u64 key = i < m ? a[i] : ~0ull;
        const int flag = i < m && key < (u64)t.n_classes && (i == 0 || a[i - 1] != key);
        int total;
        const int rank = block_scan(flag, q.red, &total);
        if (flag) {
            const int slot = s + base + rank;                                       // base + rank <= i < m
            if (slot < t.n) {
                leaf_class[slot] = (int)key;
                leaf_count[slot] = q.right[(int)key];
            } else {
                atomicOr(t.info, HSEFR_FOREST_INFO_INTERNAL);
            }
        }
        base += total;
    }
    return base;
}

struct ChooseShared {
    SearchShared search;
    unsigned short feat[MAX_D];     // 8 KB: the whole visiting order, for the visit past max_features
    int win_k[THREADS];
    double win_score[THREADS];
};

__global__ __launch_bounds__(THREADS) void choose_kernel(Work w, Sizes z, const float* x, const int* labels, int level, int force_leaf,
                                                         int* feature, double* threshold, int* left, int* right, int* weight,
                                                         int* leaf_begin, int* leaf_len, int* leaf_class, int* leaf_count, int* info) {
    __shared__ ChooseShared sh;
    const int tree = blockIdx.y, j = blockIdx.x, tid = threadIdx.x;
    const int node = level_node(w, z, tree, level, j);
    if (node < 0) return;
    const size_t at = (size_t)tree * z.M + node;
    const int s = w.node_start[at], m = w.node_len[at];
    if (s < 0 || m < 1 || s + m > z.n) {
        if (tid == 0) atomicOr(info, HSEFR_FOREST_INFO_INTERNAL);
        return;
    }
    Tree t = {x, labels, w.mult + (size_t)tree * z.n, w.rows + ((size_t)(level & 1) * z.T + tree) * z.n, z.d, z.n_classes, z.n, info};
    u64* slab = w.slab + (size_t)tree * z.mf * 2 * z.n;              // feature slot 0's: search_kernel is done with it
    u64 n_part = 0;
    for (int i = tid; i < m; i += THREADS) n_part += (u64)t.mult[checked_row(t, s + i)];
    const u64 N = block_sum(n_part, sh.search.red);
    // the winner over the features visited by search_kernel: the largest score, then the lowest slot (a slot's own ties went to
    // its lowest position)
    int win_f = -1, win_pos = 0;
    double win_thr = 0.0;
    if (!force_leaf && m >= 2) {
        const size_t slot0 = ((size_t)tree * z.W + j) * z.mf;
        int bk = -1;
        double bs = 0.0;
        for (int k = tid; k < z.mf; k += THREADS)
            if (w.cand_pos[slot0 + k] > 0 && (bk < 0 || w.cand[slot0 + k].score > bs)) bk = k, bs = w.cand[slot0 + k].score;
        sh.win_k[tid] = bk, sh.win_score[tid] = bs;
        __syncthreads();
        for (int step = THREADS / 2; step > 0; step >>= 1) {
            if (tid < step) {
                const int ok = sh.win_k[tid + step];
                const double os = sh.win_score[tid + step];
                const int mk = sh.win_k[tid];
                if (ok >= 0 && (mk < 0 || os > sh.win_score[tid] || (os == sh.win_score[tid] && ok < mk))) sh.win_k[tid] = ok, sh.win_score[tid] = os;
            }
            __syncthreads();
        }
        bk = sh.win_k[0];
        __syncthreads();
        if (bk >= 0) {
            win_f = w.order[slot0 + bk], win_pos = w.cand_pos[slot0 + bk], win_thr = w.cand[slot0 + bk].thr;
        } else if (z.mf < z.d && w.cand_pos[slot0] == 0) {       // not for a pure node: search_kernel marked it
            // no candidate among the first max_features: the visit goes on, one feature at a time (constant features; rare)
            visiting_order(sh.search.keys, z, tree, w.node_heap[at]);
            for (int k = tid; k < z.d; k += THREADS) sh.feat[k] = (unsigned short)(sh.search.keys[k] & 4095u);
            __syncthreads();
            for (int k = z.mf; k < z.d; ++k) {
                const int f = sh.feat[k];
                if (f >= z.d) break;
                const Cand c = m <= TILE ? scan_feature<true>(sh.search, t, s, m, f, slab) : scan_feature<false>(sh.search, t, s, m, f, slab);
                if (c.pure) break;
                if (c.pos > 0) {
                    win_f = f, win_pos = c.pos, win_thr = c.thr;
                    break;
                }
            }
        }
    }
    if (tid == 0) {
        feature[at] = win_f, threshold[at] = win_f >= 0 ? win_thr : 0.0, left[at] = -1, right[at] = -1, weight[at] = (int)N;
        w.split_pos[at] = win_pos;
        leaf_begin[at] = win_f >= 0 ? -1 : s;
    }
    if (win_f >= 0) {
        if (tid == 0) leaf_len[at] = -1;
        return;
    }
    // a leaf: its classes sorted, one (class, count) pair per distinct class at the segment's start in the tree's list
    const int distinct = m <= TILE ? write_leaf<true>(sh.search, t, s, m, slab, leaf_class + (size_t)tree * z.n, leaf_count + (size_t)tree * z.n)
                                   : write_leaf<false>(sh.search, t, s, m, slab, leaf_class + (size_t)tree * z.n, leaf_count + (size_t)tree * z.n);
    if (tid == 0) leaf_len[at] = distinct;
}

__global__ __launch_bounds__(THREADS) void partition_kernel(Work w, Sizes z, const float* x, int level, const int* feature,
                                                            const double* threshold, int* left, int* right, int* n_nodes, int* info) {
    __shared__ u64 red[THREADS];
    const int tree = blockIdx.y, j = blockIdx.x, tid = threadIdx.x;
    int* lb = w.level_begin + (size_t)tree * (z.D + 2);
    const int begin = lb[level], next = lb[level + 1];
    const int count = min(next, z.M) - begin;
    if (j > 0 && j >= count) return;
    // split nodes of this level before this one, and in all: where the children go
    u64 part = 0;
    for (int i = tid; i < count; i += THREADS)
        if (feature[(size_t)tree * z.M + begin + i] >= 0) part += (i < j ? 1ull : 0ull) + (1ull << 32);
    const u64 sums = block_sum(part, red);
    const int before = (int)(sums & 0xffffffffu), splits = (int)(sums >> 32);
    if (j == 0 && tid == 0) {
        const int end = next + 2 * splits;
        if (end <= z.M) {
            for (int l = level + 2; l < z.D + 2; ++l) lb[l] = end;
            n_nodes[tree] = end;
        } else {
            atomicOr(info, HSEFR_FOREST_INFO_INTERNAL);
        }
    }
    if (j >= count) return;
    const size_t at = (size_t)tree * z.M + begin + j;
    const int f = feature[at];
    if (f < 0) return;
    const int child = next + 2 * before;
    const int s = w.node_start[at], m = w.node_len[at], p = w.split_pos[at];
    if (child + 1 >= z.M || next + 2 * splits > z.M || f >= z.d || p < 1 || p >= m || s < 0 || s + m > z.n) {
        if (tid == 0) atomicOr(info, HSEFR_FOREST_INFO_INTERNAL);
        return;
    }
    if (tid == 0) {
        const size_t c = (size_t)tree * z.M + child;
        const unsigned heap = w.node_heap[at];
        left[at] = child, right[at] = child + 1;
        w.node_start[c] = s, w.node_len[c] = p, w.node_heap[c] = 2 * heap;
        w.node_start[c + 1] = s + p, w.node_len[c + 1] = m - p, w.node_heap[c + 1] = 2 * heap + 1;
    }
    const int* src = w.rows + ((size_t)(level & 1) * z.T + tree) * z.n;
    int* dst = w.rows + ((size_t)((level + 1) & 1) * z.T + tree) * z.n;
    const double thr = threshold[at];
    int lbase = 0, rbase = 0;
    for (int i0 = 0; i0 < m; i0 += THREADS) {
        const int i = i0 + tid;
        const int row = i < m ? src[s + i] : 0;
        const int go_left = i < m && (unsigned)row < (unsigned)z.n && (double)x[(size_t)row * z.d + f] <= thr;
        int total;
        const int rank = block_scan(go_left, red, &total);
        if (i < m) {
            const int to = go_left ? lbase + rank : p + rbase + (tid - rank);
            if (go_left ? to < p : to < m)
                dst[s + to] = row;
            else
                atomicOr(info, HSEFR_FOREST_INFO_INTERNAL);
        }
        lbase += total;
        rbase += min(THREADS, m - i0) - total;
    }
    if (tid == 0 && lbase != p) atomicOr(info, HSEFR_FOREST_INFO_INTERNAL);
}

struct PredictShared {
    double proba[MAX_CLASSES];
    double best[THREADS];
    int best_class[THREADS];
    int bad;
};

__global__ __launch_bounds__(THREADS) void predict_kernel(const float* q, int d, int n_classes, int n_trees, int M, int L, const int* feature,
                                                          const double* threshold, const int* left, const int* right, const int* weight,
                                                          const int* leaf_begin, const int* leaf_len, const int* leaf_class,
                                                          const int* leaf_count, double* proba, int* labels) {
    __shared__ PredictShared sh;
    const int probe = blockIdx.x, tid = threadIdx.x;
    const float* v = q + (size_t)probe * d;
    for (int c = tid; c < n_classes; c += THREADS) sh.proba[c] = 0.0;
    if (tid == 0) sh.bad = 0;
    __syncthreads();
    for (int tree = 0; tree < n_trees; ++tree) {
        const size_t nodes = (size_t)tree * M;
        int node = 0, bad = 0;
        for (int steps = 0;; ++steps) {                                             // the same walk in every thread
            const int f = feature[nodes + node];
            if (f < 0) break;
            const int next = (double)v[f < d ? f : 0] <= threshold[nodes + node] ? left[nodes + node] : right[nodes + node];
            if (f >= d || (unsigned)next >= (unsigned)M || steps >= M) {
                bad = 1;
                break;
            }
            node = next;
        }
        const int begin = leaf_begin[nodes + node], len = leaf_len[nodes + node], N = weight[nodes + node];
        if (bad || begin < 0 || len < 0 || len > L || begin > L - len || N < 1) {
            if (tid == 0) sh.bad = 1;
        } else {
            for (int i = tid; i < len; i += THREADS) {                              // a leaf's classes are distinct: no two threads meet
                const int c = leaf_class[(size_t)tree * L + begin + i];
                if ((unsigned)c < (unsigned)n_classes)
                    sh.proba[c] += (double)leaf_count[(size_t)tree * L + begin + i] / (double)N;
                else
                    sh.bad = 1;
            }
        }
        __syncthreads();
    }
    int bc = -1;
    double bv = 0.0;
    for (int c = tid; c < n_classes; c += THREADS) {
        const double p = sh.proba[c] / (double)n_trees;
        if (proba) proba[(size_t)probe * n_classes + c] = p;
        if (bc < 0 || p > bv) bc = c, bv = p;
    }
    sh.best[tid] = bv, sh.best_class[tid] = bc;
    __syncthreads();
    for (int step = THREADS / 2; step > 0; step >>= 1) {
        if (tid < step) {
            const int oc = sh.best_class[tid + step], mc = sh.best_class[tid];
            const double ov = sh.best[tid + step];
            if (oc >= 0 && (mc < 0 || ov > sh.best[tid] || (ov == sh.best[tid] && oc < mc))) sh.best_class[tid] = oc, sh.best[tid] = ov;
        }
        __syncthreads();
    }
    if (tid == 0) labels[probe] = sh.bad ? -1 : sh.best_class[0];
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
int check_sizes(const char* who, int n, int d, int n_trees, int max_depth, int max_features, Sizes* z) {
    FOREST_REQUIRE(n >= 1 && d >= 1 && n_trees >= 1 && max_depth >= 1, HSEFR_FOREST_ERR_INVALID,
                   "%s: n = %d, d = %d, n_trees = %d, max_depth = %d must all be at least 1", who, n, d, n_trees, max_depth);
    FOREST_REQUIRE(max_features >= 1 && max_features <= d, HSEFR_FOREST_ERR_INVALID, "%s: max_features = %d outside 1..d = %d", who,
                   max_features, d);
    FOREST_REQUIRE(n <= HSEFR_FOREST_MAX_N && d <= HSEFR_FOREST_MAX_D && n_trees <= HSEFR_FOREST_MAX_TREES && max_depth <= HSEFR_FOREST_MAX_DEPTH,
                   HSEFR_FOREST_ERR_UNSUPPORTED, "%s: n = %d, d = %d, n_trees = %d, max_depth = %d over the limits n <= %d, d <= %d, n_trees <= %d, "
                   "max_depth <= %d", who, n, d, n_trees, max_depth, HSEFR_FOREST_MAX_N, HSEFR_FOREST_MAX_D, HSEFR_FOREST_MAX_TREES,
                   HSEFR_FOREST_MAX_DEPTH);
    const long long full = (1ll << (max_depth + 1)) - 1, widest = 1ll << (max_depth - 1);
    z->n = n, z->d = d, z->T = n_trees, z->D = max_depth, z->mf = max_features;
    z->M = (int)(full < 2ll * n - 1 ? full : 2ll * n - 1);
    z->W = (int)(widest < n ? widest : n);
    z->n_classes = 2, z->seed = 0;
    const long long cands = (long long)n_trees * z->W * max_features;
    FOREST_REQUIRE(cands <= HSEFR_FOREST_MAX_CANDIDATES, HSEFR_FOREST_ERR_UNSUPPORTED,
                   "%s: n_trees = %d x %d nodes on the widest level x max_features = %d is %lld candidates, over the limit of %lld", who, n_trees,
                   z->W, max_features, cands, (long long)HSEFR_FOREST_MAX_CANDIDATES);
    const long long slab = n > TILE ? (long long)n_trees * max_features * 2 * n * 8 : 0;
    FOREST_REQUIRE(slab <= HSEFR_FOREST_MAX_SLAB_BYTES, HSEFR_FOREST_ERR_UNSUPPORTED,
                   "%s: n = %d rows exceed one sort tile of %d, and n_trees = %d x max_features = %d x 2 n keys of 8 bytes are %lld bytes of "
                   "sort space, over the limit of %lld", who, n, TILE, n_trees, max_features, slab, (long long)HSEFR_FOREST_MAX_SLAB_BYTES);
    return HSEFR_FOREST_OK;
}

int launched(const char* who) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", who, hipGetErrorString(e));
        return HSEFR_FOREST_ERR_HIP;
    }
    return HSEFR_FOREST_OK;
}

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int hsefr_forest_version(void) { return HSEFR_FOREST_VERSION; }

__attribute__((visibility("default"))) const char* hsefr_forest_last_error_string(void) { return g_error; }

__attribute__((visibility("default"))) size_t hsefr_forest_workspace_bytes(int n, int d, int n_trees, int max_depth, int max_features) {
    Sizes z;
    if (check_sizes("workspace_bytes", n, d, n_trees, max_depth, max_features, &z) != HSEFR_FOREST_OK) return 0;
    return layout(z, nullptr, nullptr);
}

__attribute__((visibility("default"))) int hsefr_forest_fit(const float* d_x, int n, int d, const int32_t* d_labels, int n_classes, int n_trees,
                                                             int max_depth, int max_features, int bootstrap, long long seed, int node_capacity,
                                                             int32_t* d_feature, double* d_threshold, int32_t* d_left, int32_t* d_right,
                                                             int32_t* d_weight, int32_t* d_leaf_begin, int32_t* d_leaf_len, int32_t* d_leaf_class,
                                                             int32_t* d_leaf_count, int32_t* d_n_nodes, int32_t* d_info, void* d_workspace,
                                                             size_t workspace_bytes, void* stream) {
    Sizes z;
    const int rc = check_sizes("fit", n, d, n_trees, max_depth, max_features, &z);
    if (rc != HSEFR_FOREST_OK) return rc;
    FOREST_REQUIRE(n_classes >= 2, HSEFR_FOREST_ERR_INVALID, "fit: n_classes = %d must be at least 2", n_classes);
    FOREST_REQUIRE(n_classes <= MAX_CLASSES, HSEFR_FOREST_ERR_UNSUPPORTED, "fit: n_classes = %d over the limit of %d", n_classes, MAX_CLASSES);
    FOREST_REQUIRE(bootstrap == 0 || bootstrap == 1, HSEFR_FOREST_ERR_INVALID, "fit: bootstrap = %d (0 or 1)", bootstrap);
    FOREST_REQUIRE(seed >= 0, HSEFR_FOREST_ERR_INVALID, "fit: seed = %lld must not be negative", seed);
    FOREST_REQUIRE(node_capacity == z.M, HSEFR_FOREST_ERR_INVALID,
                   "fit: node_capacity = %d, but min(2^(max_depth + 1) - 1, 2 n - 1) = %d for n = %d, max_depth = %d", node_capacity, z.M, n,
                   max_depth);
    FOREST_REQUIRE(d_x && d_labels && d_feature && d_threshold && d_left && d_right && d_weight && d_leaf_begin && d_leaf_len && d_leaf_class &&
                       d_leaf_count && d_n_nodes && d_info && d_workspace,
                   HSEFR_FOREST_ERR_INVALID, "fit: a null pointer among the inputs, the outputs or the workspace (n = %d, d = %d)", n, d);
    z.n_classes = n_classes, z.seed = (u64)seed;
    Work w;
    const size_t need = layout(z, (char*)d_workspace, &w);
    FOREST_REQUIRE(workspace_bytes >= need, HSEFR_FOREST_ERR_INVALID, "fit: workspace of %zu bytes, %zu needed (hsefr_forest_workspace_bytes)",
                   workspace_bytes, need);
    FOREST_REQUIRE(((uintptr_t)d_workspace & 15) == 0, HSEFR_FOREST_ERR_INVALID, "fit: the workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const size_t tm = (size_t)z.T * z.M, tn = (size_t)z.T * z.n;
    hipError_t e = hipMemsetAsync(d_info, 0, 4 * sizeof(int32_t), s);
    if (e == hipSuccess) e = hipMemsetAsync(w.mult, 0, tn * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_threshold, 0, tm * 8, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_leaf_count, 0, tn * 4, s);
    int32_t* minus_one[] = {d_feature, d_left, d_right, d_weight, d_leaf_begin, d_leaf_len};
    for (int32_t* p : minus_one)
        if (e == hipSuccess) e = hipMemsetAsync(p, 0xff, tm * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_leaf_class, 0xff, tn * 4, s);
    if (e != hipSuccess) {
        set_error("fit: %s", hipGetErrorString(e));
        return HSEFR_FOREST_ERR_HIP;
    }
    const dim3 block(THREADS);
    const size_t cells = (size_t)n * d;
    hipLaunchKernelGGL(validate_kernel, dim3((unsigned)((cells + THREADS - 1) / THREADS < 2048 ? (cells + THREADS - 1) / THREADS : 2048)), block, 0, s, d_x,
                       d_labels, z, d_info);
    hipLaunchKernelGGL(init_kernel, dim3((unsigned)z.T), block, 0, s, w, z, bootstrap, d_n_nodes);
    for (int level = 0; level <= z.D; ++level) {
        const long long full = 1ll << level;
        const unsigned wide = (unsigned)(full < z.n ? full : z.n);                  // the most nodes a tree can have on this level
        const dim3 nodes(wide, (unsigned)z.T);
        if (level < z.D) {
            hipLaunchKernelGGL(order_kernel, nodes, block, 0, s, w, z, level);
            hipLaunchKernelGGL(search_kernel, dim3(wide, (unsigned)z.T, (unsigned)z.mf), block, 0, s, w, z, d_x, d_labels, level, d_info);
        }
        hipLaunchKernelGGL(choose_kernel, nodes, block, 0, s, w, z, d_x, d_labels, level, level == z.D ? 1 : 0, d_feature, d_threshold, d_left,
                           d_right, d_weight, d_leaf_begin, d_leaf_len, d_leaf_class, d_leaf_count, d_info);
        if (level < z.D)
            hipLaunchKernelGGL(partition_kernel, nodes, block, 0, s, w, z, d_x, level, d_feature, d_threshold, d_left, d_right, d_n_nodes, d_info);
    }
    return launched("fit");
}

__attribute__((visibility("default"))) int hsefr_forest_predict(const float* d_q, int nq, int d, int n_classes, int n_trees, int node_capacity,
                                                                 int leaf_capacity, const int32_t* d_feature, const double* d_threshold,
                                                                 const int32_t* d_left, const int32_t* d_right, const int32_t* d_weight,
                                                                 const int32_t* d_leaf_begin, const int32_t* d_leaf_len,
                                                                 const int32_t* d_leaf_class, const int32_t* d_leaf_count, double* d_proba,
                                                                 int32_t* d_labels, void* stream) {
    FOREST_REQUIRE(nq >= 1 && d >= 1 && n_trees >= 1 && node_capacity >= 1 && leaf_capacity >= 1, HSEFR_FOREST_ERR_INVALID,
                   "predict: nq = %d, d = %d, n_trees = %d, node_capacity = %d, leaf_capacity = %d must all be at least 1", nq, d, n_trees,
                   node_capacity, leaf_capacity);
    FOREST_REQUIRE(n_classes >= 2, HSEFR_FOREST_ERR_INVALID, "predict: n_classes = %d must be at least 2", n_classes);
    FOREST_REQUIRE(nq <= HSEFR_FOREST_MAX_PROBES && d <= HSEFR_FOREST_MAX_D && n_classes <= MAX_CLASSES && n_trees <= HSEFR_FOREST_MAX_TREES,
                   HSEFR_FOREST_ERR_UNSUPPORTED, "predict: nq = %d, d = %d, n_classes = %d, n_trees = %d over the limits nq <= %d, d <= %d, "
                   "n_classes <= %d, n_trees <= %d", nq, d, n_classes, n_trees, HSEFR_FOREST_MAX_PROBES, HSEFR_FOREST_MAX_D, MAX_CLASSES,
                   HSEFR_FOREST_MAX_TREES);
    FOREST_REQUIRE((long long)n_trees * node_capacity < (1ll << 31) && (long long)n_trees * leaf_capacity < (1ll << 31), HSEFR_FOREST_ERR_UNSUPPORTED,
                   "predict: n_trees = %d x node_capacity = %d or x leaf_capacity = %d is 2^31 or more", n_trees, node_capacity, leaf_capacity);
    FOREST_REQUIRE(d_q && d_feature && d_threshold && d_left && d_right && d_weight && d_leaf_begin && d_leaf_len && d_leaf_class && d_leaf_count &&
                       d_labels,
                   HSEFR_FOREST_ERR_INVALID, "predict: a null pointer among the probes, the forest or the labels (nq = %d, d = %d)", nq, d);
    hipLaunchKernelGGL(predict_kernel, dim3((unsigned)nq), dim3(THREADS), 0, (hipStream_t)stream, d_q, d, n_classes, n_trees, node_capacity,
                       leaf_capacity, d_feature, d_threshold, d_left, d_right, d_weight, d_leaf_begin, d_leaf_len, d_leaf_class, d_leaf_count, d_proba,
                       d_labels);
    return launched("predict");
}

}  // extern "C"
