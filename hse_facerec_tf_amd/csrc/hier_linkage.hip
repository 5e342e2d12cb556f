// Average (UPGMA), complete and weighted (WPGMA) linkage on device by parallel reciprocal nearest neighbours.
//
// Replaces hac.linkage(squareform(D), method) of get_facial_clusters (facial_clustering.py:241-245) for the clustering study's
// 'average' row (facial_clustering_test.py:513) and the 'complete' / 'weighted' rows of its commented list.  Unlike single linkage these
// need the whole matrix: an fp64 n x n working copy W lives in the workspace, built from either distance source by build_working_matrix
// (hier_build.h; defined here, used by rank_order.hip too).  W is bitwise symmetric and its diagonal +inf.  All three methods are
// reducible -- d(k, i u j) >= min(d(k,i), d(k,j)) -- so every pair of clusters that are each other's nearest neighbour may merge in the
// same round; under the total order (d, lower, higher) the globally least pair is always such a pair, so every round makes progress.
// nn[i] / nnd[i] hold the least (W[i,b], b) over the other alive slots.
// A round:
//   1. pair      every alive i with nn[nn[i]] == i marks its partner; of a pair the lower slot survives, appends the record
//                (i, j, W[i,j], round) and counts one cluster down; the higher slot dies;
//   2. update    per merge (a, a') and alive column b: the new W[a,b] from the old {a, a'} x {b, b'} by the method's Lance-Williams rule
//                (b' = b's partner when b merged too: the two steps of scipy's update composed, written once by the lower survivor to
//                both W[a,b] and W[b,a]); a column whose row minimum the new entry beats is marked for a rescan.  Reads touch rows a, a'
//                and columns b' of merged pairs only, writes rows/columns of survivors x non-merged or of survivor pairs once, so no entry
//                one thread writes is read by another thread of the launch.  Dead rows and columns are left stale and masked by alive[];
//   3. finalize  survivor sizes, and the list of rows to rescan: survivors, rows whose nearest neighbour merged, marked rows;
//   4. rescan    nn / nnd of the listed rows (one workgroup per row, a grid-stride walk over the list).
// Rounds go out in batches of BATCH with no host synchronisation inside a batch; the device alive count turns rounds after completion
// into early exits, and the host reads it once per batch (rounds are not bounded by log n: a chain needs up to n - 1).  No grid-wide
// barriers, no persistent kernels.  Workspace: 8 n^2 + O(n) bytes, stream-ordered (hipMallocAsync), refused before any launch.
#include "hier_build.h"
#include "linkage_scan.h"
#ifdef HSEFR_GEOM_LIB
// Compiled a second time into libhsefr_geom.so (include/hsefr_geom.h) under this macro: the same rounds with Ward's three-term rule
// (geom_rules.h) in the update, the working matrix as first built copied out on request, and the record and clamp counts handed back.
// Without the macro this translation unit is what libhsefr.so has always compiled.
#include "geom_rules.h"
#endif

namespace hsefr {

namespace {

constexpr int BATCH = 32;          // rounds per host check of the alive count
constexpr int UPD_Y = 128;         // merges walked in parallel by the update launch (blockIdx.y)
constexpr int SCAN_BLOCKS = 1024;  // workgroups of the rescan launch

// cnt[]: 0 alive clusters, 1 merges so far, 2 first merge of the current round, 3 round number, 4 rows on the rescan list
#ifndef HSEFR_GEOM_LIB
enum { C_ALIVE = 0, C_MERGES = 1, C_RSTART = 2, C_ROUND = 3, C_LIST = 4, C_N = 5 };
#else
// 5: radicands clamped at zero.  The closest-pair engine of geom_linkage.hip hands rescan_rows a block of these words of its own
enum { C_ALIVE = 0, C_MERGES = 1, C_RSTART = 2, C_ROUND = 3, C_LIST = 4, C_CLAMPS = 5, C_N = 6 };
static_assert(C_ALIVE == HL_CNT_ALIVE && C_LIST == HL_CNT_LIST && C_N <= HL_CNT_WORDS, "hier_build.h states the rescan's two words");
#endif

__device__ __forceinline__ bool better(double v, int i, double bv, int bi) { return v < bv || (v == bv && i < bi); }

// Lance-Williams updates as scipy's _hierarchy_distance_update.pxi states them (no contraction, so the same roundings)
#ifdef HSEFR_GEOM_LIB
[[maybe_unused]]                                               // (this build's update takes geom::ward)
#endif
__device__ __forceinline__ double lw2(int method, double dx, double dy, int sx, int sy) {
#pragma clang fp contract(off)
    if (method == HSEFR_LINK_AVERAGE) return ((double)sx * dx + (double)sy * dy) / (double)(sx + sy);
    if (method == HSEFR_LINK_COMPLETE) return fmax(dx, dy);
    return 0.5 * (dx + dy);
}

// Writes a staged 32 x 32 tile s (rows R*32.., columns C*32.., C >= R) to W and its mirror.  On the diagonal tile the entry below the
// diagonal is the one above it and the diagonal itself is +inf; rows/columns past n are not written.
__device__ __forceinline__ void store_tile_sym(double (*s)[33], double* __restrict__ W, int n, int R, int C, int lane) {
    const int c = lane & 31, h = lane >> 5;
    for (int it = 0; it < 16; ++it) {
        const int r = 2 * it + h;
        const int gi = R * 32 + r, gj = C * 32 + c;
        if (gi < n && gj < n) W[(size_t)gi * n + gj] = R != C ? s[r][c] : (c > r ? s[r][c] : (c == r ? (double)INFINITY : s[c][r]));
        if (R != C) {
            const int ti = C * 32 + r, tj = R * 32 + c;
            if (ti < n && tj < n) W[(size_t)ti * n + tj] = s[c][r];
        }
    }
}

// The two build kernels take the grid ((T + 3) / 4, T) with T = ceil(n / 32) and 256 threads.
// Features: one workgroup = row tile R x column tiles 4 g .. 4 g + 3 (one per wave), only tiles with C >= R; each is one feat_tile of
// linkage_scan.h (rows on the A operand, columns on B; an inactive wave contracts nothing).
__global__ __launch_bounds__(256) void hl_build_feat_kernel(const float* __restrict__ x, int n, int d, const float* __restrict__ born,
                                                            const float* __restrict__ year, double* __restrict__ W) {
    __shared__ double s_t[4][32][33];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int T = (n + 31) / 32;
    const int R = blockIdx.y, C = blockIdx.x * 4 + wave;
    if (blockIdx.x * 4 + 3 < R) return;                        // the whole block is below the diagonal
    const bool active = C >= R && C < T;                       // wave-uniform
    const float* qp = x + (size_t)min(R * 32 + li, n - 1) * d + 4 * lh;
    float qq = 0.f;
    bool qq_done = false;
    float v[16];
    link::feat_tile(qp, x, d, min(C * 32 + li, n - 1), born, year, lh, qq, qq_done,
                    [&](int r, float& b, float& y) {
                        const int row = min(R * 32 + link::tile_row(r, lh), n - 1);
                        b = born[row];
                        y = year[row];
                    }, v, active);
#pragma unroll
    for (int r = 0; r < 16; ++r) s_t[wave][link::tile_row(r, lh)][li] = (double)v[r];
    __syncthreads();
    if (active) store_tile_sym(s_t[wave], W, n, R, C, lane);
}

// Dense: one wave = one 32 x 32 tile (R, C >= R) of the caller's matrix, read by rows into LDS and stored to both sides.
__global__ __launch_bounds__(256) void hl_build_dense_kernel(const double* __restrict__ D, int n, double* __restrict__ W) {
    __shared__ double s_t[4][32][33];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int T = (n + 31) / 32;
    const int R = blockIdx.y, C = blockIdx.x * 4 + wave;
    if (blockIdx.x * 4 + 3 < R) return;
    const bool active = C >= R && C < T;
    const int c = lane & 31, h = lane >> 5;
    for (int it = 0; active && it < 16; ++it) {
        const int r = 2 * it + h;
        const int gi = R * 32 + r, gj = C * 32 + c;
        s_t[wave][r][c] = (gi < n && gj < n) ? D[(size_t)gi * n + gj] : 0.0;
    }
    __syncthreads();
    if (active) store_tile_sym(s_t[wave], W, n, R, C, lane);
}

__global__ __launch_bounds__(256) void hl_init_kernel(int* __restrict__ alive, int* __restrict__ partner, int* __restrict__ size,
                                                      int* __restrict__ flag, int* __restrict__ list, int* __restrict__ cnt, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        alive[i] = 1;
        partner[i] = -1;
        size[i] = 1;
        flag[i] = 0;
        list[i] = i;                                         // the first scan covers every row
    }
    if (i == 0) {
        cnt[C_ALIVE] = n;
        cnt[C_MERGES] = 0;
        cnt[C_RSTART] = 0;
        cnt[C_ROUND] = 0;
        cnt[C_LIST] = n;
#ifdef HSEFR_GEOM_LIB
        cnt[C_CLAMPS] = 0;
#endif
    }
}

// Row minimum of each listed row over the other alive columns, by (value, column).  256 threads walk the row; waves reduce by shuffles,
// then through LDS.
__global__ __launch_bounds__(256) void hl_rescan_kernel(const double* __restrict__ W, int n, const int* __restrict__ alive,
                                                        const int* __restrict__ list, const int* __restrict__ cnt, int* __restrict__ nn,
                                                        double* __restrict__ nnd) {
    if (cnt[C_ALIVE] <= 1) return;
    __shared__ double s_v[4];
    __shared__ int s_i[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int rows = cnt[C_LIST];
    for (int e = blockIdx.x; e < rows; e += gridDim.x) {
        const int row = list[e];
        const double* wr = W + (size_t)row * n;
        double bv = INFINITY;
        int bi = 0x7fffffff;
        for (int b = t; b < n; b += 256) {
            const double v = wr[b];
            if (b != row && alive[b] && better(v, b, bv, bi)) { bv = v; bi = b; }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double ov = __shfl_xor(bv, m);
            const int oi = __shfl_xor(bi, m);
            if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { s_v[wave] = bv; s_i[wave] = bi; }
        __syncthreads();
        if (t == 0) {
            for (int w = 1; w < 4; ++w)
                if (better(s_v[w], s_i[w], bv, bi)) { bv = s_v[w]; bi = s_i[w]; }
            nn[row] = bi == 0x7fffffff ? -1 : bi;
            nnd[row] = bv;
        }
        __syncthreads();                                      // s_v / s_i are free for the next row
    }
}

// Every thread writes only its own partner[] / alive[] slot and reads nn[] and W only.  cnt[C_ALIVE] may drop while this runs; a thread that reads
// it at <= 1 finds every merge of the round already counted (see sl_hook_kernel).  Record slots and the count take one atomic per wave.
__global__ __launch_bounds__(256) void hl_pair_kernel(const double* __restrict__ W, int n, int* __restrict__ alive, const int* __restrict__ nn,
                                                      int* __restrict__ partner, int* __restrict__ cnt, int* __restrict__ merge_a,
                                                      int* __restrict__ merge_b, double* __restrict__ merge_h, int* __restrict__ merge_round) {
    if (*(volatile const int*)&cnt[C_ALIVE] <= 1) return;
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 256 + threadIdx.x;
    int j = -1;
    bool mutual = false;
    if (i < n && alive[i]) {
        j = nn[i];
        mutual = j >= 0 && nn[j] == i;
        partner[i] = mutual ? j : -1;
        if (mutual && j < i) alive[i] = 0;
    }
    const bool rec = mutual && i < j;
    const unsigned long long m = __ballot(rec);
    if (m == 0) return;
    const int leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) {
        base = atomicAdd(&cnt[C_MERGES], __popcll(m));
        atomicSub(&cnt[C_ALIVE], __popcll(m));
    }
    base = __shfl(base, leader);
    if (!rec) return;
    const int slot = base + __popcll(m & ((1ull << lane) - 1));
    if (slot < n - 1) {
        merge_a[slot] = i;
        merge_b[slot] = j;
        merge_h[slot] = W[(size_t)i * n + j];
        merge_round[slot] = cnt[C_ROUND];
    }
}

// blockIdx.y walks this round's merges (records cnt[C_RSTART] .. cnt[C_MERGES]), blockIdx.x * 256 + threadIdx.x is the column.
__global__ __launch_bounds__(256) void hl_update_kernel(double* __restrict__ W, int n, int method, const int* __restrict__ alive,
                                                        const int* __restrict__ partner, const int* __restrict__ size,
                                                        const int* __restrict__ nn, const double* __restrict__ nnd, int* __restrict__ flag,
                                                        int* __restrict__ cnt, const int* __restrict__ merge_a,
                                                        const int* __restrict__ merge_b) {
    if (cnt[C_ALIVE] <= 1) return;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) cnt[C_LIST] = 0;   // read again only by this round's finalize
    const int m0 = cnt[C_RSTART], m1 = min(cnt[C_MERGES], n - 1);
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n || !alive[b]) return;
    const int pb = partner[b];                                 // b's partner when b survived a merge of this round, else -1
    for (int m = m0 + blockIdx.y; m < m1; m += gridDim.y) {
        const int a = merge_a[m], a2 = merge_b[m];
        if (b == a) continue;
        const double* ra = W + (size_t)a * n;
        const double* ra2 = W + (size_t)a2 * n;
        const int sa = size[a], sa2 = size[a2];
        double v;
#ifndef HSEFR_GEOM_LIB
        if (pb < 0) {
            v = lw2(method, ra[b], ra2[b], sa, sa2);
            if (better(v, a, nnd[b], nn[b])) flag[b] = 1;
        } else {
            if (b < a) continue;                               // the lower survivor of the two writes both entries
            const double vb = lw2(method, ra[b], ra2[b], sa, sa2);       // d(a u a', b)
            const double vpb = lw2(method, ra[pb], ra2[pb], sa, sa2);    // d(a u a', b')
            v = lw2(method, vb, vpb, size[b], size[pb]);
        }
#else
        // Ward's rule also reads the merged pair's own distance.  W[a,a'] and W[b,b'] are entries of columns that died in this round's
        // pair launch: nobody writes them here.  Two pairs merged in one round compose as scipy's two steps, the lower survivor's first
        unsigned clamps = 0;
        const double daa = ra[a2];
        if (pb < 0) {
            v = geom::ward(ra[b], ra2[b], daa, sa, sa2, size[b], clamps);
            if (better(v, a, nnd[b], nn[b])) flag[b] = 1;
        } else {
            if (b < a) continue;
            const double vb = geom::ward(ra[b], ra2[b], daa, sa, sa2, size[b], clamps);       // d(a u a', b)
            const double vpb = geom::ward(ra[pb], ra2[pb], daa, sa, sa2, size[pb], clamps);   // d(a u a', b')
            v = geom::ward(vb, vpb, W[(size_t)b * n + pb], size[b], size[pb], sa + sa2, clamps);
        }
        if (clamps) atomicAdd(&cnt[C_CLAMPS], (int)clamps);
#endif
        W[(size_t)a * n + b] = v;
        W[(size_t)b * n + a] = v;
    }
}

// Sizes of the survivors and the next rescan list.  Reads partner[] of dead slots and size[] of dead slots, writes size[] of survivors.
__global__ __launch_bounds__(256) void hl_finalize_kernel(int n, const int* __restrict__ alive, const int* __restrict__ partner,
                                                          int* __restrict__ size, const int* __restrict__ nn, int* __restrict__ flag,
                                                          int* __restrict__ list, int* __restrict__ cnt) {
    if (cnt[C_ALIVE] <= 1) return;
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool want = false;
    if (i < n) {
        if (alive[i]) {
            const int p = partner[i];
            want = flag[i] != 0;
            if (p > i) {
                size[i] += size[p];
                want = true;
            } else if (nn[i] >= 0 && partner[nn[i]] >= 0) {
                want = true;                                   // its nearest neighbour merged this round
            }
        }
        flag[i] = 0;
    }
    if (i == 0) {                                              // the next round starts here; nobody else reads these in this launch
        cnt[C_RSTART] = cnt[C_MERGES];
        cnt[C_ROUND] += 1;
    }
    const unsigned long long m = __ballot(want);
    if (m == 0) return;
    const int leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(&cnt[C_LIST], __popcll(m));
    base = __shfl(base, leader);
    if (want) list[base + __popcll(m & ((1ull << lane) - 1))] = i;
}

#ifdef HSEFR_GEOM_LIB
// two threads, one count each (8-byte stores)
__global__ void hl_counts_kernel(const int* __restrict__ cnt, long long* __restrict__ counts) {
    if (threadIdx.x < 2) counts[threadIdx.x] = cnt[threadIdx.x == 0 ? C_MERGES : C_CLAMPS];
}
#endif

}  // namespace

void build_working_matrix(const DistSource& src, double* W, hipStream_t s) {
    const int T = (src.n + 31) / 32;
    const dim3 gt((T + 3) / 4, T), blk(256);
    if (src.dense)
        HSEFR_LAUNCH(hl_build_dense_kernel, gt, blk, 0, s, src.dense, src.n, W);
    else
        HSEFR_LAUNCH(hl_build_feat_kernel, gt, blk, 0, s, src.x, src.n, src.d, src.born, src.year, W);
}

#ifdef HSEFR_GEOM_LIB
void rescan_rows(const double* W, int n, const int* alive, const int* list, const int* cnt, int* nn, double* nnd, int blocks, hipStream_t s) {
    HSEFR_LAUNCH(hl_rescan_kernel, dim3(blocks), dim3(256), 0, s, W, n, alive, list, cnt, nn, nnd);
}

int launch_ward_linkage(const DistSource& src, int* merge_a, int* merge_b, double* merge_h, int* merge_round, double* w_out, long long* counts,
                        hipStream_t s) {
    const int method = 0;                                      // (the update of this build knows one rule)
#else
int launch_hier_linkage(const DistSource& src, int method, int* merge_a, int* merge_b, double* merge_h, int* merge_round, hipStream_t s) {
#endif
    const int n = src.n;
    if (n == 1) return HSEFR_OK;
    // W first (n^2 doubles), then nnd (n doubles), then int arrays: nn, alive, partner, size, flag, list, cnt
    const size_t bytes = (size_t)n * n * 8 + (size_t)n * 8 + (size_t)n * 6 * 4 + C_N * 4;
    char* ws = nullptr;
    if (hipMallocAsync((void**)&ws, bytes, s) != hipSuccess || !ws) {
        (void)hipGetLastError();
        set_error("hier_linkage: no stream-ordered workspace (%zu bytes: the %d x %d fp64 working matrix) -- too many points for this "
                  "device's free memory", bytes, n, n);
        return HSEFR_ERR_NOMEM;
    }
    double* W = (double*)ws;
    double* nnd = W + (size_t)n * n;
    int* nn = (int*)(nnd + n);
    int* alive = nn + n;
    int* partner = alive + n;
    int* size = partner + n;
    int* flag = size + n;
    int* list = flag + n;
    int* cnt = list + n;
    const dim3 blk(256), g1((n + 255) / 256);
    HSEFR_LAUNCH(hl_init_kernel, g1, blk, 0, s, alive, partner, size, flag, list, cnt, n);
    build_working_matrix(src, W, s);
#ifdef HSEFR_GEOM_LIB
    if (w_out && hipMemcpyAsync(w_out, W, (size_t)n * n * 8, hipMemcpyDeviceToDevice, s) != hipSuccess) {
        set_error("ward linkage: copying the working matrix out failed: %s", hipGetErrorString(hipGetLastError()));
        (void)hipFreeAsync(ws, s);
        return HSEFR_ERR_HIP;
    }
#endif
    const dim3 gs(n < SCAN_BLOCKS ? n : SCAN_BLOCKS), gu((n + 255) / 256, UPD_Y);
    HSEFR_LAUNCH(hl_rescan_kernel, gs, blk, 0, s, W, n, alive, list, cnt, nn, nnd);
    int rc = launch_status("hier_linkage");
    int host_cnt[2] = {n, 0};
    // every round merges at least one pair, so n - 1 rounds always suffice; the batches stop as soon as one cluster is left
    for (int done = 0; rc == HSEFR_OK && host_cnt[0] > 1 && done < n - 1; done += BATCH) {
        for (int r = 0; r < BATCH; ++r) {
            HSEFR_LAUNCH(hl_pair_kernel, g1, blk, 0, s, W, n, alive, nn, partner, cnt, merge_a, merge_b, merge_h, merge_round);
            HSEFR_LAUNCH(hl_update_kernel, gu, blk, 0, s, W, n, method, alive, partner, size, nn, nnd, flag, cnt, merge_a, merge_b);
            HSEFR_LAUNCH(hl_finalize_kernel, g1, blk, 0, s, n, alive, partner, size, nn, flag, list, cnt);
            HSEFR_LAUNCH(hl_rescan_kernel, gs, blk, 0, s, W, n, alive, list, cnt, nn, nnd);
        }
        rc = launch_status("hier_linkage");
        if (rc != HSEFR_OK || route_probe()) break;
        hipError_t e = hipMemcpyAsync(host_cnt, cnt, sizeof(host_cnt), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            set_error("hier_linkage: reading the cluster count failed: %s", hipGetErrorString(e));
            rc = HSEFR_ERR_HIP;
        }
    }
    if (rc == HSEFR_OK && !route_probe() && (host_cnt[0] != 1 || host_cnt[1] != n - 1)) {
        set_error("hier_linkage: %d clusters and %d merges left after the rounds (n=%d)", host_cnt[0], host_cnt[1], n);
        rc = HSEFR_ERR_HIP;
    }
#ifdef HSEFR_GEOM_LIB
    if (rc == HSEFR_OK && counts) {
        HSEFR_LAUNCH(hl_counts_kernel, dim3(1), dim3(64), 0, s, cnt, counts);
        rc = launch_status("ward linkage");
    }
#endif
    (void)hipFreeAsync(ws, s);
    return rc;
}

}  // namespace hsefr
