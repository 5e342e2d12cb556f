// libhsefr_geom.so (include/hsefr_geom.h): centroid, median and Ward linkage on the device -- the three methods of the clustering
// study's list (facial_clustering_test.py:514) that hsefr_hier_linkage leaves to the host.
//
// Ward is reducible, so it runs the reciprocal-nearest-neighbour rounds of hier_linkage.hip, which this library compiles a second time
// under -DHSEFR_GEOM_LIB with the three-term rule in its update (launch_ward_linkage, hier_build.h).
//
// Centroid and median are not: d(k, i u j) may be smaller than both d(k,i) and d(k,j), the tree has inversions, and two pairs that are
// each other's nearest neighbours may not merge in one round.  This file is their closest-pair engine, the primitive algorithm: n - 1
// steps, each merging the least pair under the total order (distance, lower slot, higher slot).  State: W (build_working_matrix:
// bitwise symmetric, diagonal +inf), alive[], size[], and the cached row minima nn[] / nnd[] = the least (value, column) over the alive
// columns.  A step with the pair x < y at height h = W[x,y]:
//   1. the least (nnd[r], min(r, nn[r]), max(r, nn[r])) over the rows is the pair (the row x itself holds it: nn[x] is the least column
//      among x's equal entries); the record (x, y, h, step) is written;
//   2. every other alive column i gets the rule's value at W[y,i] and W[i,y] from W[x,i], W[y,i], h and the sizes;
//   3. slot x dies, slot y takes size sx + sy;
//   4. the row minima are repaired: row y (its whole row is new) and the rows whose cached neighbour was x or y are rescanned, one
//      workgroup (LDS class: one wave) per row; any other row compares its one new entry with its cached minimum.  No step scans W.
// Two size classes:
//   n <= HSEFR_GEOM_LDS_MAX   gm_lds_kernel: ONE launch of one workgroup, W in 129 KiB of LDS (rows of 129 doubles: the column walk of
//                             step 2 touches every bank), all steps inside it between workgroup barriers -- the album case, where the
//                             launch latency of n - 1 steps would be the whole cost;
//   above                     two launches per step, enqueued back to back with no host synchronisation: gm_step_kernel (one workgroup
//                             per 256 columns; EVERY workgroup reduces nnd[] for itself, so all agree on the pair without talking) and
//                             hier_linkage.hip's rescan (rescan_rows) over the rows the step listed.
// The rule of hier_linkage.hip holds for gm_step_kernel: nothing one workgroup writes is read by another in the same launch.  What every
// workgroup reads -- nn[], nnd[], size[] -- is therefore kept twice and ping-ponged: a step reads the copies of its parity and writes
// the others (a thread writes its own column's entries).  alive[i] is read and written by column i's thread only.  The two list counts
// alternate as well: a step appends to one and its first thread clears the other, which only the previous step's rescan has read.
// W[x,.] and W[x,y] are only read; W[y,i] and W[i,y] are written by column i's thread, which alone reads W[y,i].
// No grid-wide barriers, no cooperative launches, no spin-waits, no persistent kernels.  Every store is a vector store from plain C++.
//
// Shared with the other seven libraries: no symbol (linked with -fvisibility=hidden).  What common.h declares of libhsefr.so and this
// library uses -- the error string, the route probe behind launch_status -- is defined by lib_error.h, in this source of the two.
#include <math.h>
#include <string.h>

#include "hier_build.h"
#include "geom_rules.h"
#include "lib_error.h"
#include "../../include/hsefr_geom.h"

namespace hsefr {

namespace {

constexpr int LDS_MAX = HSEFR_GEOM_LDS_MAX;
constexpr int NONE = 0x7fffffff;
constexpr int RESCAN_BLOCKS = 1024;                  // workgroups of a step's rescan launch, as the rounds': one per listed row (the rest
                                                     // leave at once), a grid-stride walk when more rows than that are listed

__device__ __forceinline__ bool better(double v, int i, double bv, int bi) { return v < bv || (v == bv && i < bi); }
__device__ __forceinline__ bool pair_better(double d, int lo, int hi, double bd, int blo, int bhi) {
    return d < bd || (d == bd && (lo < blo || (lo == blo && hi < bhi)));
}

__device__ __forceinline__ double rule(int method, double dxi, double dyi, double dxy, int sx, int sy, unsigned& clamps) {
    return method == HSEFR_GEOM_CENTROID ? geom::centroid(dxi, dyi, dxy, sx, sy, clamps) : geom::median(dxi, dyi, dxy, clamps);
}

// The workgroup's least pair (256 threads); every thread ends with it.  s_*: two sets of per-wave slots used in turn, so one barrier
// per call does (a slot is written again only behind the barrier of the call in between, which every reader has passed)
__device__ __forceinline__ void block_least_pair(double& d, int& lo, int& hi, double (*s_d)[4], int (*s_lo)[4], int (*s_hi)[4], int& turn) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const double od = __shfl_xor(d, o);
        const int olo = __shfl_xor(lo, o), ohi = __shfl_xor(hi, o);
        if (pair_better(od, olo, ohi, d, lo, hi)) {
            d = od;
            lo = olo;
            hi = ohi;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_d[turn][wave] = d;
        s_lo[turn][wave] = lo;
        s_hi[turn][wave] = hi;
    }
    __syncthreads();
    d = s_d[turn][0];
    lo = s_lo[turn][0];
    hi = s_hi[turn][0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (pair_better(s_d[turn][w], s_lo[turn][w], s_hi[turn][w], d, lo, hi)) {
            d = s_d[turn][w];
            lo = s_lo[turn][w];
            hi = s_hi[turn][w];
        }
    turn ^= 1;
}

// ---- n > LDS_MAX: two launches per step ------------------------------------------------------------------------------------------
// cnt: two blocks of HL_CNT_WORDS ints (hier_build.h: what rescan_rows reads); totals: {records written, radicands clamped}
__global__ __launch_bounds__(256) void gm_init_kernel(int* __restrict__ alive, int* __restrict__ size0, int* __restrict__ list,
                                                      int* __restrict__ cnt, unsigned long long* __restrict__ totals, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        alive[i] = 1;
        size0[i] = 1;
        list[i] = i;                                 // the first scan covers every row
    }
    if (i < 2 * HL_CNT_WORDS) cnt[i] = 0;
    __syncthreads();
    if (i == 0) {
        cnt[HL_CNT_ALIVE] = 2;                       // the rescan's early exit never applies: a step with one cluster left is not launched
        cnt[HL_CNT_WORDS + HL_CNT_ALIVE] = 2;
        cnt[HL_CNT_WORDS + HL_CNT_LIST] = n;         // the first scan reads the second block; step 0 appends to the first
    }
    if (i < 2) totals[i] = 0;                        // (a thread each: 8-byte stores)
}

__global__ __launch_bounds__(256) void gm_step_kernel(double* __restrict__ W, int n, int method, int step, int* __restrict__ alive,
                                                      const int* __restrict__ size_cur, int* __restrict__ size_next,
                                                      const int* __restrict__ nn_cur, const double* __restrict__ nnd_cur,
                                                      int* __restrict__ nn_next, double* __restrict__ nnd_next, int* __restrict__ list,
                                                      int* __restrict__ cnt_mine, int* __restrict__ cnt_other,
                                                      unsigned long long* __restrict__ totals, int* __restrict__ merge_a,
                                                      int* __restrict__ merge_b, double* __restrict__ merge_h, int* __restrict__ merge_round) {
    __shared__ double s_d[2][4];
    __shared__ int s_lo[2][4], s_hi[2][4];
    const int t = threadIdx.x;
    double h = INFINITY;
    int x = NONE, y = NONE, turn = 0;
    // (no branch around the loads: the unrolled walk keeps four rows' reads in flight; j < 0 is a dead row or one without a neighbour)
#pragma unroll 4
    for (int r = t; r < n; r += 256) {
        const int j = nn_cur[r];
        const double d = nnd_cur[r];
        const int lo = min(r, j), hi = max(r, j);
        if (j >= 0 && pair_better(d, lo, hi, h, x, y)) {
            h = d;
            x = lo;
            y = hi;
        }
    }
    block_least_pair(h, x, y, s_d, s_lo, s_hi, turn);
    const int i = blockIdx.x * 256 + t;
    const bool found = (unsigned)x < (unsigned)n && (unsigned)y < (unsigned)n && x != y;
    if (i == 0) {
        cnt_other[HL_CNT_LIST] = 0;                  // the next step's list; read last by the previous step's rescan
        if (found) {
            merge_a[step] = x;
            merge_b[step] = y;
            merge_h[step] = h;
            merge_round[step] = step;
            totals[0] += 1;
        }
    }
    if (i >= n) return;
    const double INF = (double)INFINITY;
    const int si = size_cur[i];
    if (!found) {                                    // (only a matrix of NaNs: nothing merges, the state is carried over as it is)
        size_next[i] = si;
        nn_next[i] = nn_cur[i];
        nnd_next[i] = nnd_cur[i];
        return;
    }
    if (!alive[i] || i == x) {
        if (i == x) alive[i] = 0;
        size_next[i] = si;
        nn_next[i] = -1;
        nnd_next[i] = INF;
        return;
    }
    const int sx = size_cur[x], sy = size_cur[y];
    if (i == y) {
        size_next[i] = sx + sy;
        list[atomicAdd(&cnt_mine[HL_CNT_LIST], 1)] = i;          // its whole row is new
        return;
    }
    unsigned clamps = 0;
    const double v = rule(method, W[(size_t)x * n + i], W[(size_t)y * n + i], h, sx, sy, clamps);
    W[(size_t)y * n + i] = v;
    W[(size_t)i * n + y] = v;
    size_next[i] = si;
    const int j = nn_cur[i];
    if (j == x || j == y) {
        list[atomicAdd(&cnt_mine[HL_CNT_LIST], 1)] = i;          // its cached neighbour is gone or has a new distance
    } else {
        const double bv = nnd_cur[i];
        const bool take = better(v, y, bv, j);
        nn_next[i] = take ? y : j;
        nnd_next[i] = take ? v : bv;
    }
    if (clamps) atomicAdd(&totals[1], (unsigned long long)clamps);
}

// two threads, one count each (8-byte stores)
__global__ void gm_counts_kernel(const unsigned long long* __restrict__ totals, long long* __restrict__ counts) {
    if (threadIdx.x < 2) counts[threadIdx.x] = (long long)totals[threadIdx.x];
}

// ---- n <= LDS_MAX: one launch, one workgroup, W in LDS ----------------------------------------------------------------------------
// nn / nnd of the rows s_list[0 .. *s_nlist), a wave per row; ends behind a barrier
__device__ __forceinline__ void lds_rescan(const double* s_m, int ld, int n, const int* s_alive, const int* s_list, const int* s_nlist,
                                           int* s_nn, double* s_nnd) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rows = *s_nlist;
    for (int e = wave; e < rows; e += 4) {
        const int row = s_list[e];
        double bv = INFINITY;
        int bi = NONE;
        for (int b = lane; b < n; b += 64) {
            const double v = s_m[row * ld + b];
            if (b != row && s_alive[b] && better(v, b, bv, bi)) {
                bv = v;
                bi = b;
            }
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            const double ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (better(ov, oi, bv, bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if (lane == 0) {
            s_nn[row] = bi == NONE ? -1 : bi;
            s_nnd[row] = bv;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void gm_lds_kernel(const double* __restrict__ W, int n, int method, unsigned long long* __restrict__ totals,
                                                     int* __restrict__ merge_a, int* __restrict__ merge_b, double* __restrict__ merge_h,
                                                     int* __restrict__ merge_round) {
    constexpr int LD = LDS_MAX | 1;
    __shared__ double s_m[LDS_MAX * LD];
    __shared__ double s_nnd[LDS_MAX];
    __shared__ int s_nn[LDS_MAX], s_alive[LDS_MAX], s_size[LDS_MAX], s_list[LDS_MAX];
    __shared__ int s_nlist;
    __shared__ unsigned s_clamps;
    __shared__ double s_d[2][4];
    __shared__ int s_lo[2][4], s_hi[2][4];
    const int t = threadIdx.x;
    if (n > LDS_MAX) return;                         // (a launch the host did not make)
    for (int e = t; e < n * n; e += 256) {
        const int a = e / n, b = e - a * n;
        s_m[a * LD + b] = W[e];                      // (the diagonal is +inf already)
    }
    if (t < n) {
        s_alive[t] = 1;
        s_size[t] = 1;
        s_list[t] = t;
    }
    if (t == 0) {
        s_nlist = n;
        s_clamps = 0;
    }
    __syncthreads();
    lds_rescan(s_m, LD, n, s_alive, s_list, &s_nlist, s_nn, s_nnd);
    unsigned clamps = 0;
    int turn = 0, done = 0;
    for (int step = 0; step < n - 1; ++step) {
        if (t == 0) s_nlist = 0;                     // read last by the rescan before its barrier; appended to behind the next one
        double h = INFINITY;
        int x = NONE, y = NONE;
        if (t < n) {
            const int j = s_nn[t];
            if (j >= 0) {
                h = s_nnd[t];
                x = min(t, j);
                y = max(t, j);
            }
        }
        block_least_pair(h, x, y, s_d, s_lo, s_hi, turn);
        if (!((unsigned)x < (unsigned)n && (unsigned)y < (unsigned)n && x != y)) break;      // (only a matrix of NaNs; uniform)
        if (t == 0) {
            merge_a[step] = x;
            merge_b[step] = y;
            merge_h[step] = h;
            merge_round[step] = step;
        }
        ++done;
        if (t < n && s_alive[t] && t != x) {
            if (t == y) {
                s_list[atomicAdd(&s_nlist, 1)] = t;
            } else {
                // row x and row y are read at the thread's own column; (y, t) and (t, y) are written by this thread alone
                const double v = rule(method, s_m[x * LD + t], s_m[y * LD + t], h, s_size[x], s_size[y], clamps);
                s_m[y * LD + t] = v;
                s_m[t * LD + y] = v;
                const int j = s_nn[t];
                if (j == x || j == y) {
                    s_list[atomicAdd(&s_nlist, 1)] = t;
                } else if (better(v, y, s_nnd[t], j)) {
                    s_nn[t] = y;
                    s_nnd[t] = v;
                }
            }
        }
        __syncthreads();                             // every read of the sizes and of alive[] is done
        if (t == 0) {
            s_alive[x] = 0;
            s_nn[x] = -1;
            s_size[y] += s_size[x];
        }
        __syncthreads();
        lds_rescan(s_m, LD, n, s_alive, s_list, &s_nlist, s_nn, s_nnd);
    }
    if (clamps) atomicAdd(&s_clamps, clamps);
    __syncthreads();
    if (t < 2) totals[t] = t == 0 ? (unsigned long long)done : (unsigned long long)s_clamps;      // (a thread each: 8-byte stores)
}

int geom_linkage(const DistSource& src, int method, int* merge_a, int* merge_b, double* merge_h, int* merge_round, double* w_out,
                 long long* counts, hipStream_t s) {
    HSEFR_REQUIRE(src.n >= 1, HSEFR_ERR_INVALID, "geom_linkage: n=%d", src.n);
    HSEFR_REQUIRE((src.x != nullptr) != (src.dense != nullptr), HSEFR_ERR_INVALID, "geom_linkage: pass exactly one of x and dense");
    HSEFR_REQUIRE(!src.born == !src.year, HSEFR_ERR_INVALID, "geom_linkage: born and year come together");
    HSEFR_REQUIRE(!(src.dense && src.born), HSEFR_ERR_INVALID, "geom_linkage: the age term belongs to the features path");
    HSEFR_REQUIRE(src.dense || (src.d > 0 && src.d % 8 == 0), HSEFR_ERR_INVALID, "geom_linkage: d=%d must be a positive multiple of 8", src.d);
    HSEFR_REQUIRE(method == HSEFR_GEOM_CENTROID || method == HSEFR_GEOM_MEDIAN || method == HSEFR_GEOM_WARD, HSEFR_ERR_INVALID,
                  "geom_linkage: method=%d (HSEFR_GEOM_CENTROID, _MEDIAN or _WARD)", method);
    HSEFR_REQUIRE(merge_a && merge_b && merge_h && merge_round, HSEFR_ERR_INVALID, "geom_linkage: null pointer (merge outputs)");
    const int n = src.n;
    if (counts) HSEFR_HIP_CHECK(hipMemsetAsync(counts, 0, 2 * sizeof(long long), s));
    if (n == 1) return HSEFR_OK;
    if (method == HSEFR_GEOM_WARD) return launch_ward_linkage(src, merge_a, merge_b, merge_h, merge_round, w_out, counts, s);

    // W (n^2 doubles), nnd twice, the totals, then the int arrays: nn twice, size twice, alive, list, the two count blocks
    const size_t bytes = (size_t)n * n * 8 + (size_t)n * 2 * 8 + 2 * 8 + (size_t)n * 6 * 4 + 2 * HL_CNT_WORDS * 4;
    char* ws = nullptr;
    if (hipMallocAsync((void**)&ws, bytes, s) != hipSuccess || !ws) {
        (void)hipGetLastError();
        set_error("geom_linkage: no stream-ordered workspace (%zu bytes: the %d x %d fp64 working matrix) -- too many points for this "
                  "device's free memory", bytes, n, n);
        return HSEFR_ERR_NOMEM;
    }
    double* W = (double*)ws;
    double* nnd[2] = {W + (size_t)n * n, W + (size_t)n * n + n};
    unsigned long long* totals = (unsigned long long*)(nnd[1] + n);
    int* nn[2] = {(int*)(totals + 2), (int*)(totals + 2) + n};
    int* size[2] = {nn[1] + n, nn[1] + 2 * n};
    int* alive = size[1] + n;
    int* list = alive + n;
    int* cnt[2] = {list + n, list + n + HL_CNT_WORDS};
    const dim3 blk(256), g1((n + 255) / 256);
    HSEFR_LAUNCH(gm_init_kernel, g1, blk, 0, s, alive, size[0], list, cnt[0], totals, n);
    build_working_matrix(src, W, s);
    int rc = launch_status("geom_linkage");
    if (rc == HSEFR_OK && w_out && hipMemcpyAsync(w_out, W, (size_t)n * n * 8, hipMemcpyDeviceToDevice, s) != hipSuccess) {
        set_error("geom_linkage: copying the working matrix out failed: %s", hipGetErrorString(hipGetLastError()));
        rc = HSEFR_ERR_HIP;
    }
    if (rc == HSEFR_OK && n <= LDS_MAX) {
        HSEFR_LAUNCH(gm_lds_kernel, dim3(1), blk, 0, s, W, n, method, totals, merge_a, merge_b, merge_h, merge_round);
    } else if (rc == HSEFR_OK) {
        const int blocks = n < RESCAN_BLOCKS ? n : RESCAN_BLOCKS;
        rescan_rows(W, n, alive, list, cnt[1], nn[0], nnd[0], blocks, s);                    // every row, into the copies step 0 reads
        for (int step = 0; step < n - 1; ++step) {
            const int c = step & 1, o = c ^ 1;
            HSEFR_LAUNCH(gm_step_kernel, g1, blk, 0, s, W, n, method, step, alive, size[c], size[o], nn[c], nnd[c], nn[o], nnd[o], list, cnt[c],
                         cnt[o], totals, merge_a, merge_b, merge_h, merge_round);
            if (step < n - 2) rescan_rows(W, n, alive, list, cnt[c], nn[o], nnd[o], blocks, s);
        }
    }
    if (rc == HSEFR_OK) {
        if (counts) HSEFR_LAUNCH(gm_counts_kernel, dim3(1), dim3(64), 0, s, totals, counts);
        rc = launch_status("geom_linkage");
    }
    (void)hipFreeAsync(ws, s);
    return rc;
}

}  // namespace

}  // namespace hsefr

extern "C" {

__attribute__((visibility("default"))) int hsefr_geom_version(void) { return HSEFR_GEOM_VERSION; }

__attribute__((visibility("default"))) const char* hsefr_geom_last_error(void) { return hsefr::g_error; }

__attribute__((visibility("default"))) int hsefr_geom_linkage(const float* x, int n, int d, const float* born, const float* year,
                                                              const double* dense, int method, int* merge_a, int* merge_b, double* merge_h,
                                                              int* merge_round, double* w_out, long long* counts, hsefr_stream_t stream) {
    const hsefr::DistSource src = {x, n, d, born, year, dense};
    return hsefr::geom_linkage(src, method, merge_a, merge_b, merge_h, merge_round, w_out, counts, (hipStream_t)stream);
}

}  // extern "C"
