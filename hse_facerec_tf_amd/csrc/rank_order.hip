// Rank-order face clustering on device: the rankorder_clustering branch of get_facial_clusters (facial_clustering.py:214-285; the
// parameterised find_clusters of facial_clustering_test.py:23-239, whose zero guard on the normalised distance is followed here) with
// the reference's clusters, on hier_build.h's fp64 n x n working matrix W (features or a caller's dense matrix; the diagonal counts as 0).
//
// Slots are faces; a cluster lives in its lowest slot, which is its smallest face index, so ties by slot are ties by the reference's
// cluster position.  NB = 20 list entries, KN = 12 of them in the normalisation.  Once per call:
//   topk      per alive row the first min(NB, clusters) alive columns by (W[row, col], col) -> lidx / lval; the first pass also leaves
//             T[row] = the sum of the first min(KN, n) list values, added in list order.  One wave per row, four rows per workgroup: the
//             row is streamed with 16-byte loads against the wave's running threshold (the current NB-th best), so most elements cost
//             one compare; the few that pass go to a 128-entry LDS list that is ranked down to NB whenever it could overflow.
// then per iteration:
//   pair      one wave per cluster a, for every b != a of a's list: nd = (1 / ((T[a] + T[b]) / k / (|a| + |b|))) * C[a,b] (0 when the
//             mean is 0) against norm_threshold, then the two asymmetric rank orders from the 20 x 20 compare of the two lists against
//             rank_threshold; an accepted pair is united at once (lock-free union by CAS, the higher root under the lower);
//   flatten   root[] of every alive slot, the new label of every face, members per root, the new cluster count (the one value the host
//             reads per iteration: an unchanged count ends the call);
//   key/order the members of every root that grew, in ascending slot order: position = the number of merged slots with a smaller
//             (root, slot), counted by one wave per slot -- no atomics, so the order is the same on every run;
//   merge     per root that grew: T[root] += T[member] in ascending member order (the fixed summation order; the reference's own follows
//             Python set iteration), sizes, alive[member] = 0;
//   rows      W[root, c] = min over the root's members of W[member, c] for every column c.  Thread (root, c) reads column c of its own
//             members' rows and writes W[root, c]; member sets are disjoint, so no thread reads what another thread of the launch writes;
//   cols      W[r, root] = min over members of W[r, member] for every alive row r.  Thread (r, root) reads row r at its own members'
//             columns and writes W[r, root]: again disjoint.  Dead rows and columns keep stale values and are masked by alive[];
//   topk      on the alive rows.
// A sequence of threshold pairs keeps a second copy of W and of the first lists (both are threshold-independent) and restores them by
// device copies.  No grid-wide barriers, no persistent kernels.  Workspace 8 n^2 (16 n^2 for a sequence) + O(n NB) bytes,
// stream-ordered, refused before any launch.
#include "hier_build.h"

namespace hsefr {

namespace {

constexpr int NB = 20;             // neighbour list entries
constexpr int KN = 12;             // of which the normalisation sums
constexpr int CAP = 128;           // LDS candidates per wave: NB kept + two appends of at most 64
constexpr int ROW_Y = 1024;        // grid.y of the row reduce

typedef double f64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bool better(double v, int i, double bv, int bi) { return v < bv || (v == bv && i < bi); }

__global__ __launch_bounds__(256) void ro_init_kernel(unsigned char* __restrict__ alive, int* __restrict__ fsize, int* __restrict__ lab,
                                                      int* __restrict__ parent, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        alive[i] = 1;
        fsize[i] = 1;
        lab[i] = i;
        parent[i] = i;
    }
}

// Ranks the wave's m <= CAP candidates by (value, column) and keeps the first NB, sorted, at the head of the list.  Every lane has read
// the whole list before any lane writes (one wave, LDS operations in program order).
__device__ __attribute__((noinline)) void ro_rank(double* __restrict__ sv, int* __restrict__ sc, int m) {
    const int lane = threadIdx.x & 63;
    const double v0 = lane < m ? sv[lane] : 0.0, v1 = lane + 64 < m ? sv[lane + 64] : 0.0;
    const int c0 = lane < m ? sc[lane] : 0, c1 = lane + 64 < m ? sc[lane + 64] : 0;
    int r0 = 0, r1 = 0;
    for (int j = 0; j < m; ++j) {
        const double vj = sv[j];
        const int cj = sc[j];
        r0 += better(vj, cj, v0, c0);
        r1 += better(vj, cj, v1, c1);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < m && r0 < NB) { sv[r0] = v0; sc[r0] = c0; }
    if (lane + 64 < m && r1 < NB) { sv[r1] = v1; sc[r1] = c1; }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ... and the NB-th becomes the threshold (by value through the noinline call: nothing of the caller's lives in scratch)
__device__ __forceinline__ void ro_compact(double* __restrict__ sv, int* __restrict__ sc, int& cnt, double& tv, int& tc) {
    ro_rank(sv, sc, cnt);
    cnt = cnt < NB ? cnt : NB;
    if (cnt == NB) { tv = sv[NB - 1]; tc = sc[NB - 1]; }
}

// One element of the row: appended when it beats the threshold and its column is alive (live).  cnt, tv, tc are wave-uniform.
__device__ __forceinline__ void ro_offer(double v, int col, bool live, double* __restrict__ sv, int* __restrict__ sc, int& cnt, double& tv,
                                         int& tc) {
    const int lane = threadIdx.x & 63;
    if (__ballot(live && better(v, col, tv, tc)) == 0) return;
    if (cnt + 64 > CAP) ro_compact(sv, sc, cnt, tv, tc);
    const bool pass = live && better(v, col, tv, tc);
    const unsigned long long mask = __ballot(pass);
    if (pass) {
        const int pos = cnt + __popcll(mask & ((1ull << lane) - 1));
        sv[pos] = v;
        sc[pos] = col;
    }
    cnt += __popcll(mask);
}

// FIRST: every slot is alive (alive[] is not read) and T[row] is written.  Otherwise the alive flags of a pair travel with its load, so
// that no element waits for a second trip to memory.
template <bool FIRST>
__global__ __launch_bounds__(256) void ro_topk_kernel(const double* __restrict__ W, int n, const unsigned char* __restrict__ alive, int len,
                                                      int kn, int* __restrict__ lidx, double* __restrict__ lval, double* __restrict__ T) {
    __shared__ double s_v[4][CAP];
    __shared__ int s_c[4][CAP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * 4 + wave;
    if (row >= n || (!FIRST && !alive[row])) return;           // wave-uniform; the waves of a workgroup never meet at a barrier
    double* sv = s_v[wave];
    int* sc = s_c[wave];
    int cnt = 0, tc = 0x7fffffff;
    double tv = INFINITY;
    const size_t base = (size_t)row * n;
    const int e0 = (int)(base & 1);                            // columns e0, e0 + 2, ... start 16-byte aligned pairs
    const int pairs = (n - e0) >> 1;
    const f64x2* wp = (const f64x2*)(W + base + e0);
    // the unpaired head and tail columns
    {
        const int col = lane == 0 ? 0 : n - 1;
        const bool in = (lane == 0 && e0 == 1) || (lane == 1 && e0 + 2 * pairs < n);
        double v = in ? W[base + col] : 0.0;
        if (col == row) v = 0.0;
        ro_offer(v, col, in && (FIRST || alive[col]), sv, sc, cnt, tv, tc);
    }
    for (int p0 = 0; p0 < pairs; p0 += 256) {
        f64x2 v[4];
        bool l0[4], l1[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int p = p0 + u * 64 + lane;
            const bool in = p < pairs;
            v[u] = in ? wp[p] : f64x2{0.0, 0.0};
            l0[u] = in && (FIRST || alive[e0 + 2 * p]);
            l1[u] = in && (FIRST || alive[e0 + 2 * p + 1]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int col = e0 + 2 * (p0 + u * 64 + lane);
            if (col == row) v[u][0] = 0.0;
            if (col + 1 == row) v[u][1] = 0.0;
            ro_offer(v[u][0], col, l0[u], sv, sc, cnt, tv, tc);
            ro_offer(v[u][1], col + 1, l1[u], sv, sc, cnt, tv, tc);
        }
    }
    ro_compact(sv, sc, cnt, tv, tc);
    if (lane < len) {
        const bool have = lane < cnt;                          // cnt == len: the alive columns number at least len
        lidx[(size_t)row * NB + lane] = have ? sc[lane] : -1;
        lval[(size_t)row * NB + lane] = have ? sv[lane] : INFINITY;
    }
    if (FIRST && lane == 0) {
        double s = 0.0;
        for (int j = 0; j < kn && j < cnt; ++j) s += sv[j];
        T[row] = s;
    }
}

__device__ __forceinline__ int ro_find(int* parent, int x) {
    int p;
    while ((p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != x) x = p;
    return x;
}

// The higher root goes under the lower; a lost race starts again from the new roots.  Roots only ever point lower, so the root of a
// finished component is its lowest slot whatever the order of the unions.
__device__ __forceinline__ void ro_unite(int* parent, int a, int b) {
    for (;;) {
        a = ro_find(parent, a);
        b = ro_find(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        if (atomicCAS(&parent[hi], hi, lo) == hi) return;
    }
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// O(a,b) of the reference from pos = the position of this lane's entry of a's list in b's list (-1: absent): the walk stops after the
// first entry that heads b's list -> (penalty, entries walked)
__device__ __forceinline__ void ro_asym(int pos, int len, int& pen, int& walked) {
    const int lane = threadIdx.x & 63;
    const unsigned long long z = __ballot(pos == 0);
    const int stop = z ? __ffsll((long long)z) - 1 : len;
    walked = z ? stop + 1 : len;
    pen = wave_sum(lane < stop && pos > 0 ? pos : 0);
}

__global__ __launch_bounds__(256) void ro_pair_kernel(int n, const unsigned char* __restrict__ alive, int len, double k, double norm_thr,
                                                      double rank_thr, const int* __restrict__ lidx, const double* __restrict__ lval,
                                                      const double* __restrict__ T, const int* __restrict__ fsize, int* parent) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int a = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (a >= n || !alive[a]) return;
    const bool on = lane < len;
    const int la = on ? lidx[(size_t)a * NB + lane] : -1;
    const double va = on ? lval[(size_t)a * NB + lane] : 0.0;
    const double Ta = T[a];
    const int sa = fsize[a];
    for (int e = 0; e < len; ++e) {
        const int b = __shfl(la, e);
        if (b == a || b < 0) continue;
        const double cab = __shfl(va, e);
        const double mean = (Ta + T[b]) / k / (double)(sa + fsize[b]);
        const double nd = mean != 0.0 ? (1.0 / mean) * cab : 0.0;
        if (nd >= norm_thr) continue;
        const int lb = on ? lidx[(size_t)b * NB + lane] : -2;
        int pa = -1, pb = -1;                                   // of la in b's list, of lb in a's list
        for (int j = 0; j < len; ++j) {
            const int eb = __shfl(lb, j), ea = __shfl(la, j);
            if (on && eb == la) pa = j;
            if (on && ea == lb) pb = j;
        }
        int pen_ab, n_ab, pen_ba, n_ba;
        ro_asym(pa, len, pen_ab, n_ab);
        ro_asym(pb, len, pen_ba, n_ba);
        const double ro = (double)(pen_ab + pen_ba) / (double)(n_ab < n_ba ? n_ab : n_ba);
        if (ro >= rank_thr) continue;
        if (lane == 0) ro_unite(parent, a, b);
    }
}

// cnt[0] = clusters after this iteration.  parent[] is complete (the previous launch) and only read here.
__global__ __launch_bounds__(256) void ro_flatten_kernel(int n, const unsigned char* __restrict__ alive, int* parent, int* __restrict__ root,
                                                         int* __restrict__ lab, int* __restrict__ msize, int* __restrict__ cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool is_root = false;
    if (i < n) {
        lab[i] = ro_find(parent, lab[i]);
        if (alive[i]) {
            const int r = ro_find(parent, i);
            root[i] = r;
            atomicAdd(&msize[r], 1);
            is_root = r == i;
        }
    }
    const unsigned long long m = __ballot(is_root);
    if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(&cnt[0], __popcll(m));
}

// key[i] = the root of a slot whose cluster grew in this iteration, -1 for every other slot; parent[] is made ready for the next one
__global__ __launch_bounds__(256) void ro_key_kernel(int n, const unsigned char* __restrict__ alive, const int* __restrict__ root,
                                                     const int* __restrict__ msize, int* __restrict__ key, int* __restrict__ parent) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    key[i] = alive[i] && msize[root[i]] > 1 ? root[i] : -1;
    parent[i] = i;
}

// One wave per merged slot i: members[pos] = i with pos = the number of merged slots before it by (root, slot); a root is the first
// of its members, and remembers where they start.
__global__ __launch_bounds__(256) void ro_order_kernel(int n, const int* __restrict__ key, int* __restrict__ members, int* __restrict__ moff) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int ki = key[i];
    if (ki < 0) return;
    int before = 0;
    for (int j = lane; j < n; j += 64) {
        const int kj = key[j];
        before += kj >= 0 && (kj < ki || (kj == ki && j < i));
    }
    before = wave_sum(before);
    if (lane == 0) {
        members[before] = i;
        if (ki == i) moff[i] = before;
    }
}

// One wave per root that grew: T and the face count take the members' in ascending slot order, and the members die.
__global__ __launch_bounds__(256) void ro_merge_kernel(int n, const int* __restrict__ key, const int* __restrict__ members,
                                                       const int* __restrict__ moff, const int* __restrict__ msize, double* __restrict__ T,
                                                       int* __restrict__ fsize, unsigned char* __restrict__ alive) {
    const int lane = threadIdx.x & 63;
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= n || key[s] != s) return;
    const int off = moff[s], cntm = msize[s];
    double t = T[s];
    int f = fsize[s];
    for (int c0 = 1; c0 < cntm; c0 += 64) {
        const int here = min(64, cntm - c0);
        const int m = lane < here ? members[off + c0 + lane] : s;
        const double tm = lane < here ? T[m] : 0.0;
        const int fm = lane < here ? fsize[m] : 0;
        if (lane < here) alive[m] = 0;
        for (int l = 0; l < here; ++l) t += __shfl(tm, l);
        f += wave_sum(fm);
    }
    if (lane == 0) {
        T[s] = t;
        fsize[s] = f;
    }
}

__global__ __launch_bounds__(256) void ro_rows_kernel(double* __restrict__ W, int n, const int* __restrict__ key, const int* __restrict__ members,
                                                      const int* __restrict__ moff, const int* __restrict__ msize) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    for (int s = blockIdx.y; s < n; s += gridDim.y) {
        if (key[s] != s || c >= n) continue;
        const int off = moff[s], cntm = msize[s];
        double v = W[(size_t)s * n + c];
#pragma unroll 4
        for (int e = 1; e < cntm; ++e) {
            const double w = W[(size_t)members[off + e] * n + c];
            v = w < v ? w : v;
        }
        W[(size_t)s * n + c] = v;
    }
}

__global__ __launch_bounds__(256) void ro_cols_kernel(double* __restrict__ W, int n, const unsigned char* __restrict__ alive,
                                                      const int* __restrict__ key, const int* __restrict__ members,
                                                      const int* __restrict__ moff, const int* __restrict__ msize) {
    for (int r = blockIdx.x; r < n; r += gridDim.x) {
        if (!alive[r]) continue;
        double* wr = W + (size_t)r * n;
        for (int s = threadIdx.x; s < n; s += 256) {
            if (key[s] != s) continue;
            const int off = moff[s], cntm = msize[s];
            double v = wr[s];
#pragma unroll 4
            for (int e = 1; e < cntm; ++e) {
                const double w = wr[members[off + e]];
                v = w < v ? w : v;
            }
            wr[s] = v;
        }
    }
}

size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

}  // namespace

int launch_rank_order(const DistSource& src, const double* thresholds, int pairs, int* labels, int* iterations, hipStream_t s) {
    const int n = src.n;
    const bool keep = pairs > 1;                               // a sequence keeps the matrix and the first lists
    const size_t nn = (size_t)n * n * 8, lv = up16((size_t)n * NB * 8), li = up16((size_t)n * NB * 4), nd = up16((size_t)n * 8),
                 ni = up16((size_t)n * 4 + 16);
    // W [W0] lval [lval0] T [T0] lidx [lidx0] fsize lab parent root key members moff (msize, cnt) alive
    const size_t bytes = up16(nn) * (keep ? 2 : 1) + (lv + li + nd) * (keep ? 2 : 1) + ni * 8 + up16((size_t)n);
    char* ws = nullptr;
    if (hipMallocAsync((void**)&ws, bytes, s) != hipSuccess || !ws) {
        (void)hipGetLastError();
        set_error("rank_order: no stream-ordered workspace (%zu bytes: %s%d x %d fp64 working matri%s) -- too many faces for this "
                  "device's free memory", bytes, keep ? "two " : "the ", n, n, keep ? "ces" : "x");
        return HSEFR_ERR_NOMEM;
    }
    char* p = ws;
    auto take = [&p](size_t b) { char* q = p; p += b; return q; };
    double* W = (double*)take(up16(nn));
    double* W0 = keep ? (double*)take(up16(nn)) : W;
    double* lval = (double*)take(lv);
    double* lval0 = keep ? (double*)take(lv) : lval;
    double* T = (double*)take(nd);
    double* T0 = keep ? (double*)take(nd) : T;
    int* lidx = (int*)take(li);
    int* lidx0 = keep ? (int*)take(li) : lidx;
    int* fsize = (int*)take(ni);
    int* lab = (int*)take(ni);
    int* parent = (int*)take(ni);
    int* root = (int*)take(ni);
    int* key = (int*)take(ni);
    int* members = (int*)take(ni);
    int* moff = (int*)take(ni);
    int* msize = (int*)take(ni);
    int* cnt = msize + n;                                      // cleared with msize
    unsigned char* alive = (unsigned char*)take(up16((size_t)n));

    const dim3 blk(256), g1((n + 255) / 256), gw((n + 3) / 4);
    const dim3 gr((n + 255) / 256, n < ROW_Y ? n : ROW_Y), gc(n);
    const int kn = n < KN ? n : KN;                            // min(KN, min(NB, n))

    HSEFR_LAUNCH(ro_init_kernel, g1, blk, 0, s, alive, fsize, lab, parent, n);
    build_working_matrix(src, W0, s);
    HSEFR_LAUNCH(ro_topk_kernel<true>, gw, blk, 0, s, W0, n, alive, n < NB ? n : NB, kn, lidx0, lval0, T0);
    int rc = launch_status("rank_order");
    hipError_t e = hipSuccess;
    for (int t = 0; rc == HSEFR_OK && t < pairs; ++t) {
        const double norm_thr = thresholds[2 * t], rank_thr = thresholds[2 * t + 1];
        if (!route_probe() && keep) {
            if (t > 0) HSEFR_LAUNCH(ro_init_kernel, g1, blk, 0, s, alive, fsize, lab, parent, n);
            e = hipMemcpyAsync(W, W0, nn, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipMemcpyAsync(lval, lval0, (size_t)n * NB * 8, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipMemcpyAsync(lidx, lidx0, (size_t)n * NB * 4, hipMemcpyDeviceToDevice, s);
            if (e == hipSuccess) e = hipMemcpyAsync(T, T0, (size_t)n * 8, hipMemcpyDeviceToDevice, s);
        }
        int prev = n, iters = 0;
        // every iteration but the last lowers the count, so n + 1 always suffice
        while (rc == HSEFR_OK && e == hipSuccess && iters <= n) {
            const int len = prev < NB ? prev : NB;
            if (iters > 0) HSEFR_LAUNCH(ro_topk_kernel<false>, gw, blk, 0, s, W, n, alive, len, kn, lidx, lval, T);
            ++iters;
            if (!route_probe()) e = hipMemsetAsync(msize, 0, (size_t)(n + 1) * 4, s);
            HSEFR_LAUNCH(ro_pair_kernel, gw, blk, 0, s, n, alive, len, (double)kn, norm_thr, rank_thr, lidx, lval, T, fsize, parent);
            HSEFR_LAUNCH(ro_flatten_kernel, g1, blk, 0, s, n, alive, parent, root, lab, msize, cnt);
            rc = launch_status("rank_order");
            int now = prev;
            if (rc == HSEFR_OK && !route_probe() && e == hipSuccess) {
                e = hipMemcpyAsync(&now, cnt, sizeof(int), hipMemcpyDeviceToHost, s);
                if (e == hipSuccess) e = hipStreamSynchronize(s);
            }
            if (rc != HSEFR_OK || e != hipSuccess || (now == prev && !route_probe())) break;
            HSEFR_LAUNCH(ro_key_kernel, g1, blk, 0, s, n, alive, root, msize, key, parent);
            HSEFR_LAUNCH(ro_order_kernel, gw, blk, 0, s, n, key, members, moff);
            HSEFR_LAUNCH(ro_merge_kernel, gw, blk, 0, s, n, key, members, moff, msize, T, fsize, alive);
            HSEFR_LAUNCH(ro_rows_kernel, gr, blk, 0, s, W, n, key, members, moff, msize);
            HSEFR_LAUNCH(ro_cols_kernel, gc, blk, 0, s, W, n, alive, key, members, moff, msize);
            if (route_probe()) break;
            prev = now;
        }
        if (rc == HSEFR_OK && e == hipSuccess && !route_probe())
            e = hipMemcpyAsync(labels + (size_t)t * n, lab, (size_t)n * 4, hipMemcpyDeviceToDevice, s);
        if (iterations) iterations[t] = iters;
    }
    if (rc == HSEFR_OK && e != hipSuccess) {
        set_error("rank_order: a copy or the read of the cluster count failed: %s", hipGetErrorString(e));
        rc = HSEFR_ERR_HIP;
    }
    (void)hipFreeAsync(ws, s);
    return rc;
}

}  // namespace hsefr
