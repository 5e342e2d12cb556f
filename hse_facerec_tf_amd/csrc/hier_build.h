// The fp64 n x n working matrix shared by hier_linkage.hip (average / complete / weighted linkage) and rank_order.hip, from one of two
// sources:
//   features  W[i,j] = w(i,j) of linkage.hip (the fp32 MFMA contraction, the same fragment row norms, the optional age term, clipped at
//             0) widened to fp64; each 32 x 32 tile of the upper triangle is computed once and stored to both sides through LDS;
//   dense     a caller's fp64 D [n,n], read as its upper triangle D[min(i,j), max(i,j)] (what squareform(D, checks=False) reads),
//             copied to both sides; the caller's buffer is never written.
// W is bitwise symmetric and its diagonal +inf.  Both kernels take the grid ((T + 3) / 4, T) with T = ceil(n / 32) and 256 threads.
#pragma once
#include "common.h"

namespace hsefr {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

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

// Features: one workgroup = row tile R x column tiles 4 g .. 4 g + 3 (one per wave), only tiles with C >= R.  The contraction, the norms
// and the epilogue are sl_row_min_feat_kernel's (rows on the A operand, columns on B).
__global__ __launch_bounds__(256) void hl_build_feat_kernel(const float* __restrict__ x, int n, int d, const float* __restrict__ born,
                                                            const float* __restrict__ year, double* __restrict__ W) {
    __shared__ double s_t[4][32][33];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int T = (n + 31) / 32;
    const int R = blockIdx.y, C = blockIdx.x * 4 + wave;
    if (blockIdx.x * 4 + 3 < R) return;                        // the whole block is below the diagonal
    const bool active = C >= R && C < T;                       // wave-uniform
    const bool age = born != nullptr;
    const float* qp = x + (size_t)min(R * 32 + li, n - 1) * d + 4 * lh;
    const int gcol = C * 32 + li;
    const float* gp = x + (size_t)min(gcol, n - 1) * d + 4 * lh;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float gg = 0.f, qs = 0.f;
    for (int k = 0; active && k < d; k += 8) {
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
    const float qq = qs + __shfl_xor(qs, 32);
    const float gb = age ? born[min(gcol, n - 1)] : 0.f, gy = age ? year[min(gcol, n - 1)] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int rr = (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float s = __shfl(qq, rr) + gg;
        float v = sqrtf(fmaxf(fmaf(-2.f, acc[r], s), 0.f));
        if (age) {
            const int row = min(R * 32 + rr, n - 1);
            const float br = born[row], yr = year[row];
            const float t = gb - br;
            const float den = 2.f * fmaxf(yr, gy) - (br + gb);
            v = fmaxf(v + 0.1f * (t * t) / den, 0.f);
        }
        s_t[wave][rr][li] = (double)v;
    }
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

}  // namespace
}  // namespace hsefr
