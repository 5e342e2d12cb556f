// Row scans of the distance graph shared by linkage.hip (single linkage) and dbscan.hip, and the one definition of the clustering
// distance w(i,j) that every clustering kernel reads.  Two sources (a DistSource of common.h):
//   features  w(i,j) = max(sqrt(max(|x_i|^2 + |x_j|^2 - 2 x_i.x_j, 0)) + 0.1 (born_j - born_i)^2 / (2 max(year_i, year_j) - born_i - born_j), 0)
//             (the age term only with born / year), the contraction on the fp32 MFMA (mfma_dot.h, as in nn1_kernel) -- every w(i,j) is
//             computed by the same commutative expression from the same row norms and the same FMA chain whichever side of a tile i falls
//             on, so the graph is bitwise symmetric.  feat_tile below is the only place that expression is written: the row scans here
//             and the working matrix of hier_build.h (average / complete / weighted linkage, rank-order) both call it, so the distances
//             are the same bits in every clustering method (tests/test_hier_linkage_gpu.py compares the two families' global minimum);
//   dense     a caller's fp64 D [n,n], read as its upper triangle D[min(i,j), max(i,j)] (what squareform(D, checks=False) reads).
// Each kernel built on them keeps its own selection and reduction.
#pragma once
#include "common.h"
#include "mfma_dot.h"

namespace hsefr {
namespace link {

typedef unsigned long long u64;

template <typename T>
__device__ __forceinline__ bool better(T v, int i, T bv, int bi) { return v < bv || (v == bv && i < bi); }

// the tile row of accumulator r in half-wave lh
__device__ __forceinline__ int tile_row(int r, int lh) { return (r & 3) + 8 * (r >> 2) + 4 * lh; }

// One 32 x 32 feature tile: v[r] = w(row tile_row(r, lh) of the tile's 32 rows, point grow), lane (li, lh) holding column li = its own
// grow.  qp / x + grow d + 4 lh are mfma_dot_32x32's operands (rows on A, columns on B).  Row norms come from the fragments that feed the
// MFMAs: lane (li, lh) sums the same elements in the same order for a row on either operand, and the halves meet in a commutative add,
// so |x_i|^2 is one value whichever side i is on.  qq (lane t holds |x|^2 of tile row t) is taken from this tile unless qq_done says
// the caller already holds it: the rows are the same for every tile of a row scan.  row_age(r, born, year) gives the ages of tile row r
// and is called only with an age term (born != nullptr).
template <typename RowAge>
__device__ __forceinline__ void feat_tile(const float* qp, const float* x, int d, int grow, const float* born, const float* year, int lh,
                                          float& qq, bool& qq_done, RowAge row_age, float (&v)[16], bool on = true) {
    const bool age = born != nullptr;
    const float gb = age ? born[grow] : 0.f, gy = age ? year[grow] : 0.f;
    f32x16 acc;
    float gg, qs;
    mfma_dot_32x32(qp, x + (size_t)grow * d + 4 * lh, d, acc, qs, gg, on);
    gg += __shfl_xor(gg, 32);
    if (!qq_done) { qq = qs + __shfl_xor(qs, 32); qq_done = true; }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float s = __shfl(qq, tile_row(r, lh)) + gg;
        float w = sqrtf(fmaxf(fmaf(-2.f, acc[r], s), 0.f));
        if (age) {
            float br, yr;
            row_age(r, br, yr);
            const float t = gb - br;
            const float den = 2.f * fmaxf(yr, gy) - (br + gb);
            w = fmaxf(w + 0.1f * (t * t) / den, 0.f);
        }
        v[r] = w;
    }
}

// Features: one workgroup = 32 rows x all n columns, its 4 waves take column tiles of 32 round-robin (nn1_kernel's layout).  Lane
// (li, lh) holds the 16 accumulator rows row(r) of the 32 x 32 tile and column li.  The rows' ages are read once, their norms on the
// wave's first tile.
struct FeatScan {
    const float* x;
    const float* born;
    const float* year;
    const float* qp;
    int n, d, q0, lh;
    float born_r[16], year_r[16];
    float qq = 0.f;          // |x_row|^2 (lane rr holds row q0 + rr), from the wave's first tile
    bool qq_done = false;

    __device__ __forceinline__ FeatScan(const float* x_, int n_, int d_, const float* born_, const float* year_)
        : x(x_), born(born_), year(year_), n(n_), d(d_), q0(blockIdx.x * 32), lh((threadIdx.x & 63) >> 5) {
        const bool age = born != nullptr;
        qp = x + (size_t)min(q0 + (int)(threadIdx.x & 31), n - 1) * d + 4 * lh;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = row(r);
            born_r[r] = age ? born[i] : 0.f;
            year_r[r] = age ? year[i] : 0.f;
        }
    }
    // the tile row of accumulator r, and its point (clamped: rows past n repeat the last one and are never stored)
    __device__ __forceinline__ int rr(int r) const { return tile_row(r, lh); }
    __device__ __forceinline__ int row(int r) const { return min(q0 + rr(r), n - 1); }

    // v[r] = w(row(r), grow)
    __device__ __forceinline__ void tile(int grow, float (&v)[16]) {
        feat_tile(qp, x, d, grow, born, year, lh, qq, qq_done, [this](int r, float& b, float& y) { b = born_r[r]; y = year_r[r]; }, v);
    }
};

// Dense fp64: one workgroup = 64 rows x all n columns, walked in 64 x 64 tiles of the UPPER triangle staged through LDS with coalesced
// row reads -- tile (R, C) with C > R is read as it is, C < R from its mirror D[C, R] and transposed, C == R by (min, max).  Thread t
// holds row t / 4 and the columns t % 4 + 4 m of each tile.  Bandwidth-bound: every upper element is read twice per scan.
// Stage tile (r0, c0) into s_t (callers put a barrier on each side).
__device__ __forceinline__ void dense_stage(const double* __restrict__ D, int n, int r0, int c0, double (*s_t)[65]) {
    const int t = threadIdx.x;
    const int sr0 = c0 < r0 ? c0 : r0, sc0 = c0 < r0 ? r0 : c0;
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int a = (t >> 6) + 4 * k, b = t & 63;
        const int gr = sr0 + a, gc = sc0 + b;
        s_t[a][b] = (gr < n && gc < n) ? D[(size_t)gr * n + gc] : 0.0;
    }
}

// w(r0 + ri, c0 + cj) from the staged tile
__device__ __forceinline__ double dense_at(const double (*s_t)[65], int r0, int c0, int ri, int cj) {
    const bool up = c0 > r0 || (c0 == r0 && ri < cj);
    return up ? s_t[ri][cj] : s_t[cj][ri];
}

}  // namespace link

// Boruvka rounds (linkage.hip) over the edges of one source: afterwards label[] (inside ws) holds every vertex's component root.  With
// core == nullptr every edge is a candidate (single linkage: the minimum spanning tree, its n - 1 edges written to edge_*); otherwise an
// edge is one only if both ends are core and w <= eps (features: compared as w <= eps_f, the largest float <= eps), and edge_* may be
// null.  ws holds boruvka_bytes(n); nothing is synchronised.
size_t boruvka_bytes(int n);
int* boruvka_rounds(const DistSource& src, const unsigned char* core, float eps_f, double eps, char* ws, int* edge_a, int* edge_b,
                    double* edge_h, hipStream_t s);

}  // namespace hsefr
