// libhsefr_split.so (include/hsefr_split.h): the same-photo split of EVERY cluster of a clustering in one pass on the device -- the
// reference's rule that two faces of one photo are two people (facial_clustering.py:247-259), which clustering._split_groups runs
// cluster by cluster on the host.
//
// A group is a list of points (members[offsets[g] .. offsets[g + 1])); its k x k matrix is P[a][b] = w(m_a, m_b) + penalty * [same photo],
// and its answer is complete linkage on P cut at `cut`.  w(i,j) is linkage_scan.h's: feat_tile, the one definition of the clustering
// distance, called here with GATHERED operands (its row pointer and its column index are per lane already, so no row is copied), or the
// caller's dense[min(i,j), max(i,j)].  The flags this file is compiled with are libhsefr.so's (csrc/build.sh), so the bits are the ones
// the clusters were formed by.
//
// Launches of a call, whatever the number of groups:
//   split_build_kernel   one wave per 32 x 32 tile of a group's upper triangle; a workgroup finds its (group, tile row, tile column) from
//                        the groups' first_tile prefix (mixed_frames.hip finds its frame the same way).  The tile goes through LDS to
//                        both sides of the group's matrix in the slab (and of dist_out), penalty added, diagonal +inf; a wave that saw
//                        an entry above `cut` ORs a bit into the group's flag word (not a maximum of double bits: dense entries may be
//                        negative).
//   split_chain_kernel   one workgroup per group, three instances by size, chosen on the host from the offsets: up to 32 members one wave
//                        with the matrix in 8 KiB of LDS (the workgroup IS the wave: its barriers cost nothing), up to 128 a workgroup of
//                        256 with the matrix in 129 KiB of LDS (rows of 129: a column walk touches every bank), above that a workgroup of
//                        256 on the slab itself.  A workgroup first checks its members against [0, n) (a bad one: sublabels -1, counted,
//                        nothing else read), then takes the early answer -- one member, or no entry above `cut`: one cluster, exact since
//                        complete linkage's heights are monotone and the last is the largest entry -- and only then runs the chain.
// The chain is clustering.complete_linkage_labels, step for step: the nearest-neighbour chain from the lowest live slot, the row minimum
// by the total order better(value, index) of linkage_scan.h with the previous chain element winning a tie, the merged cluster kept in
// the higher slot with the plain fp64 maximum of the two rows, the chain kept across merges.  It is sequential and latency-bound; the
// parallelism is the groups and, inside one, the row minimum and the row update.  A merge at or below `cut` relabels the lower slot's
// component to the higher slot's at once: by reducibility a cluster made above `cut` never merges at or below it again, so the
// components at the end are the union-find's.  They are numbered by first occurrence with a ballot scan.
// Every store is a vector store from plain C++.
//
// Shared with the other six libraries: no symbol (linked with -fvisibility=hidden).  What common.h declares of libhsefr.so and this file
// uses -- the error string, the route probe behind launch_status -- is defined by lib_error.h for this library alone.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "linkage_scan.h"
#include "lib_error.h"
#include "../../include/hsefr_split.h"

namespace hsefr {

namespace {

constexpr int WAVE_MAX = HSEFR_SPLIT_WAVE_MAX, LDS_MAX = HSEFR_SPLIT_LDS_MAX;
constexpr int ABOVE_CUT = 1;                         // a group's flag word

// what the kernels read of a group (uploaded by the call)
struct GroupRow {                                    // 32 bytes
    long long off;                                   // its first member
    long long dist;                                  // the first element of its k x k matrix in the slab and in dist_out
    int k, first_tile, tiles, reserved;              // members; the prefix of tiles * (tiles + 1) / 2; ceil(k / 32), 0 for k == 1
};
static_assert(sizeof(GroupRow) == 32, "table layout");

// the last group whose first_tile is at most `block` (first_tile ascends from 0; a group without tiles shares its value with the next)
__device__ __forceinline__ int group_of_block(const GroupRow* __restrict__ rows, int groups, int block) {
    int lo = 0, hi = groups;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rows[mid].first_tile <= block)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int safe_member(int m, int n) { return (unsigned)m < (unsigned)n ? m : 0; }

// p[0] = v0 and, with `both`, p[1] = v1: one 16-byte store where p is 16-byte aligned (a group's rows are, when k and its place in the
// slab are even), two 8-byte stores otherwise
typedef double f64x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void store_pair(double* p, double v0, double v1, bool both) {
    if (both && ((uintptr_t)p & 15) == 0) {
        *reinterpret_cast<f64x2*>(p) = f64x2{v0, v1};
        asm volatile("s_nop 1" ::: "memory");        // gfx950 store-data hazard: two wait states behind a 16-byte store (tools/isa_lint.py)
    } else {
        p[0] = v0;
        if (both) p[1] = v1;
    }
}

__global__ __launch_bounds__(64) void split_build_kernel(const float* __restrict__ x, int n, int d, const float* __restrict__ born,
                                                         const float* __restrict__ year, const double* __restrict__ dense,
                                                         const int* __restrict__ members, const GroupRow* __restrict__ rows, int groups,
                                                         const int* __restrict__ photo, double penalty, double cut,
                                                         double* __restrict__ slab, double* __restrict__ dist_out, int* __restrict__ flags) {
    __shared__ double s_t[32][33];
    const int lane = threadIdx.x, li = lane & 31, lh = lane >> 5;
    const int g = group_of_block(rows, groups, (int)blockIdx.x);
    const GroupRow gr = rows[g];
    const int k = gr.k, T = gr.tiles;
    int t = (int)blockIdx.x - gr.first_tile, R = 0;
    while (R < T - 1 && t >= T - R) {                // row R of the upper triangle holds T - R tiles
        t -= T - R;
        ++R;
    }
    const int C = R + t;
    if (T < 1 || C >= T) return;                     // (a table the host did not build)
    const int* mem = members + gr.off;
    // lane li holds the point of the tile's row li and of its column li; rows and columns past k repeat the last member and are not
    // stored; a member outside [0, n) reads point 0 instead (its group is answered with -1 by the chain kernel, whatever is built here)
    const int mr = safe_member(mem[min(R * 32 + li, k - 1)], n), mc = safe_member(mem[min(C * 32 + li, k - 1)], n);
    if (x) {
        float qq = 0.f;
        bool qq_done = false;
        float v[16];
        link::feat_tile(x + (size_t)mr * d + 4 * lh, x, d, mc, born, year, lh, qq, qq_done,
                        [&](int r, float& b, float& y) {
                            const int row = __shfl(mr, link::tile_row(r, lh));
                            b = born[row];
                            y = year[row];
                        }, v);
#pragma unroll
        for (int r = 0; r < 16; ++r) s_t[link::tile_row(r, lh)][li] = (double)v[r];
    } else {
        for (int it = 0; it < 16; ++it) {
            const int r = 2 * it + lh;
            const int i = __shfl(mr, r);
            s_t[r][li] = dense[(size_t)min(i, mc) * n + max(i, mc)];
        }
    }
    __syncthreads();
    const int pr = photo[mr], pc = photo[mc];
    double* out = slab + gr.dist;
    double* out2 = dist_out ? dist_out + gr.dist : nullptr;
    // a lane stores two neighbouring columns of a row, 16 lanes a tile row, 4 rows per step
    const int c0 = (lane & 15) * 2;
    const int pr0 = __shfl(pr, c0), pr1 = __shfl(pr, c0 + 1), pc0 = __shfl(pc, c0), pc1 = __shfl(pc, c0 + 1);
    bool above = false;
    for (int it = 0; it < 8; ++it) {
        const int r = 4 * it + (lane >> 4);
        const int pa = __shfl(pr, r), pm = __shfl(pc, r);
        const int a = R * 32 + r, b = C * 32 + c0;
        if (a < k && b < k) {
            double p[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int c = c0 + q;
                p[q] = (double)INFINITY;
                if (a != b + q) {
                    const double w = (R != C || c > r) ? s_t[r][c] : s_t[c][r];
                    p[q] = pa == (q ? pc1 : pc0) ? w + penalty : w;
                    above |= b + q < k && p[q] > cut;
                }
            }
            store_pair(out + (size_t)a * k + b, p[0], p[1], b + 1 < k);
            if (out2) store_pair(out2 + (size_t)a * k + b, p[0], p[1], b + 1 < k);
        }
        if (R != C) {                                 // the mirror: (column tile's point r, row tile's point c) = s_t[c][r]
            const int ti = C * 32 + r, tj = R * 32 + c0;
            if (ti < k && tj < k) {
                const double w0 = s_t[c0][r], w1 = s_t[c0 + 1][r];
                const double p0 = pm == pr0 ? w0 + penalty : w0, p1 = pm == pr1 ? w1 + penalty : w1;
                store_pair(out + (size_t)ti * k + tj, p0, p1, tj + 1 < k);
                if (out2) store_pair(out2 + (size_t)ti * k + tj, p0, p1, tj + 1 < k);
            }
        }
    }
    if (__any(above) && lane == 0) atomicOr(&flags[g], ABOVE_CUT);
}

// the workgroup's minimum of (v, i) by better(); every thread ends with it.  s_rv / s_ri: two sets of per-wave slots used in turn, so
// one barrier per call does (a slot is written again only behind the barrier of the call in between, which every reader has passed)
template <int THREADS>
__device__ __forceinline__ void block_argmin(double& v, int& i, double (*s_rv)[4], int (*s_ri)[4], int& turn) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const double ov = __shfl_xor(v, o);
        const int oi = __shfl_xor(i, o);
        if (link::better(ov, oi, v, i)) {
            v = ov;
            i = oi;
        }
    }
    if (THREADS > 64) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) {
            s_rv[turn][wave] = v;
            s_ri[turn][wave] = i;
        }
        __syncthreads();
        v = s_rv[turn][0];
        i = s_ri[turn][0];
#pragma unroll
        for (int w = 1; w < THREADS / 64; ++w)
            if (link::better(s_rv[turn][w], s_ri[turn][w], v, i)) {
                v = s_rv[turn][w];
                i = s_ri[turn][w];
            }
        turn ^= 1;
    }
}

// KMAX > 0: groups of at most KMAX members, the matrix and the three word arrays in LDS; KMAX == 0: any size, on the slab and on `words`
template <int KMAX, int THREADS>
__global__ __launch_bounds__(THREADS) void split_chain_kernel(const int* __restrict__ members, int n, const GroupRow* __restrict__ rows,
                                                              const int* __restrict__ list, const int* __restrict__ flags, double* slab,
                                                              int* words, long long total, double cut, int* __restrict__ sublabel,
                                                              unsigned long long* stats) {
    constexpr bool IN_LDS = KMAX > 0;
    constexpr int LD = KMAX | 1;
    __shared__ double s_m[IN_LDS ? KMAX * LD : 1];
    __shared__ int s_w[IN_LDS ? 3 * KMAX : 1];
    __shared__ double s_rv[2][4];
    __shared__ int s_ri[2][4];
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x;
    const GroupRow gr = rows[list[blockIdx.x]];
    const int k = gr.k;
    const int* mem = members + gr.off;
    int* lab = sublabel + gr.off;
    if (IN_LDS && k > KMAX) return;                  // (a table the host did not build)

    int bad = 0;
    for (int j0 = 0; j0 < k; j0 += THREADS) {
        const int j = j0 + tid;
        bad += __syncthreads_count(j < k && (unsigned)mem[j] >= (unsigned)n);
    }
    if (bad) {
        for (int j = tid; j < k; j += THREADS) lab[j] = -1;
        if (tid == 0 && stats) atomicAdd(&stats[HSEFR_SPLIT_STAT_BAD], (unsigned long long)bad);
        return;
    }
    if (k == 1 || !(flags[list[blockIdx.x]] & ABOVE_CUT)) {
        for (int j = tid; j < k; j += THREADS) lab[j] = 0;
        if (tid == 0 && stats) atomicAdd(&stats[HSEFR_SPLIT_STAT_EARLY], 1ull);
        return;
    }

    const double INF = (double)INFINITY;
    double* M;
    int ld;
    int *chain, *alive, *comp;
    if (IN_LDS) {
        const double* src = slab + gr.dist;
        for (int e = tid; e < k * k; e += THREADS) {
            const int a = e / k, b = e - a * k;
            s_m[a * LD + b] = src[e];                // (the diagonal is +inf already)
        }
        M = s_m;
        ld = LD;
        chain = s_w;
        alive = s_w + KMAX;
        comp = s_w + 2 * KMAX;
    } else {
        M = slab + gr.dist;
        ld = k;
        chain = words + gr.off;
        alive = words + total + gr.off;
        comp = words + 2 * total + gr.off;
    }
    for (int j = tid; j < k; j += THREADS) {
        alive[j] = 1;
        comp[j] = j;
    }
    __syncthreads();

    int len = 0, first = 0, turn = 0;
    for (int m = 0; m < k - 1; ++m) {
        int xx, yp;                                  // the chain's top and the element below it (-1: none)
        if (len == 0) {
            while (first < k - 1 && !alive[first]) ++first;
            xx = first;
            yp = -1;
            len = 1;
            if (tid == 0) chain[0] = xx;
        } else {
            xx = chain[len - 1];
            yp = len > 1 ? chain[len - 2] : -1;
        }
        double h;
        for (;;) {
            const double* row = M + (size_t)xx * ld;
            const double cur = yp >= 0 ? row[yp] : INF;
            double bv = INF;
            int bi = 0x7fffffff;
            for (int j = tid; j < k; j += THREADS) {
                const double v = row[j];
                if (link::better(v, j, bv, bi)) {
                    bv = v;
                    bi = j;
                }
            }
            block_argmin<THREADS>(bv, bi, s_rv, s_ri, turn);
            int y = bv < cur ? bi : yp;
            bool forced = false;
            if (y < 0) {
                // only with entries that are not finite (a row of +inf or NaN): the lowest live slot other than the top, so that the
                // loop ends and every index stays inside the group
                for (y = 0; y < k - 1 && (!alive[y] || y == xx); ++y) {}
                forced = true;
            }
            if (!forced && len > 1 && y == yp) {
                h = cur;
                break;
            }
            if (forced || len >= k) {                 // (a chain of k elements cannot grow: the same kind of input) merge, start afresh
                h = row[y];
                __syncthreads();                      // (the update below rewrites that entry)
                yp = y;
                len = 2;
                break;
            }
            if (tid == 0) chain[len] = y;
            ++len;
            yp = xx;
            xx = y;
        }
        len -= 2;
        const int a = min(xx, yp), b = max(xx, yp);
        // the merged cluster lives on in slot b with the larger of the two rows; slot a dies.  Entries (a, b), (b, a), (a, a), (b, b) are
        // written with +inf by more than one thread, and read only by threads that replace what they read with +inf
        double* ra = M + (size_t)a * ld;
        double* rb = M + (size_t)b * ld;
        const bool join = h <= cut;
        for (int j = tid; j < k; j += THREADS) {
            double tmax = fmax(ra[j], rb[j]);
            if (j == a || j == b) tmax = INF;
            rb[j] = tmax;
            M[(size_t)j * ld + b] = tmax;
            ra[j] = INF;
            M[(size_t)j * ld + a] = INF;
            if (join && comp[j] == a) comp[j] = b;
        }
        if (tid == 0) alive[a] = 0;
        __syncthreads();
    }

    // components -> labels 0 .. c - 1 by first occurrence: the first point of each (kept where the chain was), the leaders' ranks by a
    // ballot scan (kept where the live flags were)
    int* firstp = chain;
    int* rank = alive;
    for (int j = tid; j < k; j += THREADS) firstp[j] = 0x7fffffff;
    __syncthreads();
    for (int j = tid; j < k; j += THREADS) atomicMin(&firstp[comp[j]], j);
    __syncthreads();
    int running = 0;
    for (int j0 = 0; j0 < k; j0 += THREADS) {
        const int p = j0 + tid;
        const bool lead = p < k && firstp[comp[p]] == p;
        const unsigned long long bal = __ballot(lead);
        const int lane = tid & 63, wave = tid >> 6;
        int pre = __popcll(bal & ((1ull << lane) - 1ull));
        int tot = __popcll(bal);
        if (THREADS > 64) {
            if (lane == 0) s_cnt[wave] = tot;
            __syncthreads();
            tot = 0;
#pragma unroll
            for (int w = 0; w < THREADS / 64; ++w) {
                if (w < wave) pre += s_cnt[w];
                tot += s_cnt[w];
            }
            __syncthreads();
        }
        if (lead) rank[p] = running + pre;
        running += tot;
    }
    __syncthreads();
    for (int j = tid; j < k; j += THREADS) lab[j] = rank[firstp[comp[j]]];
    if (tid == 0 && stats) {
        atomicAdd(&stats[IN_LDS ? HSEFR_SPLIT_STAT_LDS : HSEFR_SPLIT_STAT_GLOBAL], 1ull);
        atomicAdd(&stats[HSEFR_SPLIT_STAT_MERGES], (unsigned long long)(k - 1));
    }
}

// host scratch of a call (malloc, not std::vector: the library exports its three entries and nothing of the C++ runtime's templates)
struct HostBytes {
    unsigned char* p;
    explicit HostBytes(size_t n) : p((unsigned char*)malloc(n ? n : 1)) {}
    ~HostBytes() { free(p); }
    HostBytes(const HostBytes&) = delete;
    HostBytes& operator=(const HostBytes&) = delete;
};

int split_groups(const DistSource& src, const int* members, const long long* offsets, int groups, const int* photo, double penalty,
                 double cut, int* sublabel, double* dist_out, long long* stats, hipStream_t s) {
    HSEFR_REQUIRE(src.n >= 1, HSEFR_ERR_INVALID, "split_groups: n=%d", src.n);
    HSEFR_REQUIRE((src.x != nullptr) != (src.dense != nullptr), HSEFR_ERR_INVALID, "split_groups: pass exactly one of x and dense");
    HSEFR_REQUIRE(!src.born == !src.year, HSEFR_ERR_INVALID, "split_groups: born and year come together");
    HSEFR_REQUIRE(!(src.dense && src.born), HSEFR_ERR_INVALID, "split_groups: the age term belongs to the features path");
    HSEFR_REQUIRE(src.dense || (src.d > 0 && src.d % 8 == 0), HSEFR_ERR_INVALID, "split_groups: d=%d must be a positive multiple of 8", src.d);
    HSEFR_REQUIRE(members && offsets && photo && sublabel, HSEFR_ERR_INVALID, "split_groups: null %s pointer",
                  !members ? "members" : (!offsets ? "offsets" : (!photo ? "photo" : "sublabel")));
    HSEFR_REQUIRE(groups >= 0, HSEFR_ERR_INVALID, "split_groups: groups=%d", groups);
    HSEFR_REQUIRE(isfinite(penalty) && penalty >= 0, HSEFR_ERR_INVALID, "split_groups: penalty=%g must be finite and >= 0", penalty);
    HSEFR_REQUIRE(isfinite(cut), HSEFR_ERR_INVALID, "split_groups: cut=%g must be finite", cut);
    HSEFR_REQUIRE(offsets[0] == 0, HSEFR_ERR_INVALID, "split_groups: the offsets start at %lld, not at 0", offsets[0]);
    for (int g = 0; g < groups; ++g) {
        HSEFR_REQUIRE(offsets[g + 1] > offsets[g], HSEFR_ERR_INVALID,
                      "split_groups: the offsets do not strictly increase (group %d: %lld, then %lld)", g, offsets[g], offsets[g + 1]);
        HSEFR_REQUIRE(offsets[g + 1] < (1ll << 31), HSEFR_ERR_INVALID, "split_groups: the offsets reach %lld at group %d (2^31 members or more)",
                      offsets[g + 1], g);
    }
    if (groups == 0) return HSEFR_OK;

    // the table: the groups' rows, then the groups listed class by class
    const size_t table_bytes = (size_t)groups * (sizeof(GroupRow) + sizeof(int));
    HostBytes table(table_bytes);
    HSEFR_REQUIRE(table.p, HSEFR_ERR_NOMEM, "split_groups: out of host memory for the table of %d groups", groups);
    GroupRow* rows = (GroupRow*)table.p;
    int* list = (int*)(table.p + (size_t)groups * sizeof(GroupRow));
    const long long total = offsets[groups];
    long long elems = 0, tiles = 0;
    int count[3] = {0, 0, 0};
    for (int g = 0; g < groups; ++g) {
        const long long k = offsets[g + 1] - offsets[g];
        GroupRow& r = rows[g];
        r.off = offsets[g];
        r.dist = elems;
        r.k = (int)k;
        r.first_tile = (int)tiles;
        r.tiles = k > 1 ? (int)((k + 31) / 32) : 0;
        r.reserved = 0;
        elems += k * k;
        tiles += (long long)r.tiles * (r.tiles + 1) / 2;
        HSEFR_REQUIRE(tiles < (1ll << 31), HSEFR_ERR_UNSUPPORTED, "split_groups: %lld tiles or more: too many", tiles);
        ++count[k <= WAVE_MAX ? 0 : (k <= LDS_MAX ? 1 : 2)];
    }
    int at[3] = {0, count[0], count[0] + count[1]};
    for (int g = 0; g < groups; ++g) {
        const int k = rows[g].k;
        list[at[k <= WAVE_MAX ? 0 : (k <= LDS_MAX ? 1 : 2)]++] = g;
    }

    // one allocation: the slab, the table, the flag words, and the word arrays of the chains that run outside LDS
    const size_t slab_bytes = (size_t)elems * sizeof(double);
    const size_t flag_bytes = (size_t)groups * sizeof(int);
    const size_t word_bytes = count[2] ? (size_t)total * 3 * sizeof(int) : 0;
    const size_t bytes = slab_bytes + table_bytes + flag_bytes + word_bytes;
    char* ws = nullptr;
    if (hipMallocAsync((void**)&ws, bytes, s) != hipSuccess || !ws) {
        (void)hipGetLastError();
        set_error("split_groups: no stream-ordered workspace (%zu bytes: %lld matrix entries of %d groups, fp64) -- too much for this device's "
                  "free memory", bytes, elems, groups);
        return HSEFR_ERR_NOMEM;
    }
    double* slab = (double*)ws;
    const GroupRow* d_rows = (const GroupRow*)(ws + slab_bytes);
    const int* d_list = (const int*)(ws + slab_bytes + (size_t)groups * sizeof(GroupRow));
    int* d_flags = (int*)(ws + slab_bytes + table_bytes);
    int* d_words = (int*)(ws + slab_bytes + table_bytes + flag_bytes);
    unsigned long long* d_stats = (unsigned long long*)stats;
    hipError_t e = hipMemcpyAsync(ws + slab_bytes, table.p, table_bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_flags, 0, flag_bytes, s);
    if (e == hipSuccess && stats) e = hipMemsetAsync(stats, 0, HSEFR_SPLIT_STATS * sizeof(long long), s);
    int rc = HSEFR_OK;
    if (e == hipSuccess) {
        if (tiles)
            HSEFR_LAUNCH(split_build_kernel, dim3((unsigned)tiles), dim3(64), 0, s, src.x, src.n, src.d, src.born, src.year, src.dense, members,
                         d_rows, groups, photo, penalty, cut, slab, dist_out, d_flags);
        if (count[0])
            HSEFR_LAUNCH((split_chain_kernel<WAVE_MAX, 64>), dim3((unsigned)count[0]), dim3(64), 0, s, members, src.n, d_rows, d_list, d_flags,
                         slab, d_words, total, cut, sublabel, d_stats);
        if (count[1])
            HSEFR_LAUNCH((split_chain_kernel<LDS_MAX, 256>), dim3((unsigned)count[1]), dim3(256), 0, s, members, src.n, d_rows,
                         d_list + count[0], d_flags, slab, d_words, total, cut, sublabel, d_stats);
        if (count[2])
            HSEFR_LAUNCH((split_chain_kernel<0, 256>), dim3((unsigned)count[2]), dim3(256), 0, s, members, src.n, d_rows,
                         d_list + count[0] + count[1], d_flags, slab, d_words, total, cut, sublabel, d_stats);
        rc = launch_status("split_groups");
    }
    const hipError_t e_free = hipFreeAsync(ws, s);
    if (e == hipSuccess) e = e_free;
    if (e != hipSuccess) {
        set_error("split_groups: %s", hipGetErrorString(e));
        return HSEFR_ERR_HIP;
    }
    return rc;
}

}  // namespace

}  // namespace hsefr

extern "C" {

__attribute__((visibility("default"))) int hsefr_split_version(void) { return HSEFR_SPLIT_VERSION; }

__attribute__((visibility("default"))) const char* hsefr_split_last_error(void) { return hsefr::g_error; }

__attribute__((visibility("default"))) int hsefr_split_groups(const float* x, int n, int d, const float* born, const float* year,
                                                              const double* dense, const int* members, const long long* offsets_host,
                                                              int groups, const int* photo, double penalty, double cut, int* sublabel,
                                                              double* dist_out, long long* stats, hsefr_stream_t stream) {
    const hsefr::DistSource src = {x, n, d, born, year, dense};
    return hsefr::split_groups(src, members, offsets_host, groups, photo, penalty, cut, sublabel, dist_out, stats, (hipStream_t)stream);
}

}  // extern "C"
