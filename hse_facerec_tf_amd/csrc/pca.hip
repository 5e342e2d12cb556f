// PCA on the device for the '+PCA' identification pipelines (facerec_test.py:269-273, 417-432): hsefr_pca_fit / hsefr_pca_transform.
//
// fit:  fp64 column means -> fp64 covariance C [d,d] of the centred fp32 rows -> the k largest eigenpairs of C by blocked subspace
// iteration on b = k + oversampling vectors (no library eigensolver on this path):
//     Z = C Q + sigma Q ; Q = orthonormalise(Z)                   every iteration (CholeskyQR: Gram, Cholesky, triangular solve)
//     T = Q^T (C + sigma) Q ; T = V theta V^T ; Q <- Q V           at convergence checks only (Rayleigh-Ritz; one-sided Jacobi)
// until |C v_i - lambda_i v_i| <= 1e-10 lambda_1 for every i < k.  sigma = 2^-16 trace(C) / d shifts the spectrum away from zero: the
// eigenvectors are C's, lambda = theta - sigma, and a rank-deficient C (a constant column, n - 1 < d, zero padding) still gives a
// block Z of full rank, which CholeskyQR needs.  The vectors are stored as ROWS (Qt [b,d]), so every product is out[i][j] = sum_k
// A(i,k) B(j,k) over operands given by two strides each -- one MFMA tile kernel (v_mfma_f64_16x16x4_f64) serves the covariance, C Q, the
// Gram and Rayleigh-Ritz matrices, the rotations and hsefr_pca_transform.  Everything is deterministic: fixed summation orders, a
// counter-based start block, no floating-point atomics.  Steps that need the whole grid are separate launches; the host reads eight
// bytes per convergence check.
#include "common.h"

namespace hsefr {
namespace {

typedef double pca_f64x4 __attribute__((ext_vector_type(4)));

// ---- the product kernel ----------------------------------------------------------------------------------------------------------
// element (row r, summation index k) of an operand = p[r * sr + k * sk]: fp64, or (with `mean`) fp32 minus mean[feature], where the
// feature is the index whose stride is 1.  Rows >= rows and k >= K read as zero.
struct PcaOperand {
    const void* p;
    long long sr, sk;
    int rows;
    const double* mean;
};
// out[i][j] = alpha * acc (+ *sigma * add[i][j]) for i < M, j < ncols (ncols may exceed the B operand's rows: those columns are zero).
// sym: M == N and the result is symmetric -- only tiles that touch j >= i are computed, and every value goes to [i][j] and [j][i].
struct PcaEpilogue {
    void* out;
    long long ldo;
    int f32out, ncols, sym;
    double alpha;
    const double* sigma;
    const double* add;
};

constexpr int PCA_TM = 32, PCA_TN = 64, PCA_TK = 16;

__device__ __forceinline__ double pca_op_load(const PcaOperand& o, int r, int k, int K) {
    if (r >= o.rows || k >= K) return 0.0;
    const long long at = (long long)r * o.sr + (long long)k * o.sk;
    if (o.mean) return (double)((const float*)o.p)[at] - o.mean[o.sk == 1 ? k : r];
    return ((const double*)o.p)[at];
}

// a [R rows][PCA_TK] tile, R * 16 / 256 elements per thread, the fastest thread index along the operand's unit stride
template <int R>
__device__ __forceinline__ void pca_tile_load(const PcaOperand& o, int r0, int k0, int K, int tid, double (&v)[R / 16]) {
#pragma unroll
    for (int e = 0; e < R / 16; ++e) {
        const int idx = tid + 256 * e;
        const int r = o.sk == 1 ? idx / PCA_TK : idx % R, k = o.sk == 1 ? idx % PCA_TK : idx / R;
        v[e] = pca_op_load(o, r0 + r, k0 + k, K);
    }
}
template <int R>
__device__ __forceinline__ void pca_tile_store(const PcaOperand& o, double (*s)[R + 1], int tid, const double (&v)[R / 16]) {
#pragma unroll
    for (int e = 0; e < R / 16; ++e) {
        const int idx = tid + 256 * e;
        const int r = o.sk == 1 ? idx / PCA_TK : idx % R, k = o.sk == 1 ? idx % PCA_TK : idx / R;
        s[k][r] = v[e];
    }
}

// 256 threads = 4 waves, a 32 x 64 output tile: wave w owns rows 16 (w & 1) .. and columns 32 (w >> 1) .. (two 16 x 16 MFMA tiles).
// Lane l supplies A[row l & 15][k = l >> 4] and B[k = l >> 4][column l & 15]; result register r of lane l is row (l >> 4) + 4 r,
// column l & 15 (the f64 map, not the f32 one).
__global__ __launch_bounds__(256) void pca_gemm_kernel(PcaOperand A, PcaOperand B, int M, int K, PcaEpilogue ep) {
    __shared__ double As[PCA_TK][PCA_TM + 1];
    __shared__ double Bs[PCA_TK][PCA_TN + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * PCA_TM, n0 = blockIdx.y * PCA_TN;
    if (ep.sym && n0 + PCA_TN - 1 < m0) return;               // wholly below the diagonal: its mirror tile writes it
    const int wm = (wave & 1) * 16, wn = (wave >> 1) * 32;
    const int r = lane & 15, q = lane >> 4;
    pca_f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    double va[PCA_TM / 16], vb[PCA_TN / 16];
    pca_tile_load<PCA_TM>(A, m0, 0, K, tid, va);
    pca_tile_load<PCA_TN>(B, n0, 0, K, tid, vb);
    for (int k0 = 0; k0 < K; k0 += PCA_TK) {
        __syncthreads();                                      // the previous tile has been read
        pca_tile_store<PCA_TM>(A, As, tid, va);
        pca_tile_store<PCA_TN>(B, Bs, tid, vb);
        __syncthreads();
        if (k0 + PCA_TK < K) {                                // the next tile travels while this one is multiplied
            pca_tile_load<PCA_TM>(A, m0, k0 + PCA_TK, K, tid, va);
            pca_tile_load<PCA_TN>(B, n0, k0 + PCA_TK, K, tid, vb);
        }
#pragma unroll
        for (int kk = 0; kk < PCA_TK; kk += 4) {
            const double a = As[kk + q][wm + r];
            const double b0 = Bs[kk + q][wn + r], b1 = Bs[kk + q][wn + 16 + r];
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1, acc1, 0, 0, 0);
        }
    }
    const double sig = ep.sigma ? *ep.sigma : 0.0;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const pca_f64x4 acc = t ? acc1 : acc0;
        const int j = n0 + wn + 16 * t + r;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int i = m0 + wm + q + 4 * g;
            if (i >= M || j >= ep.ncols || (ep.sym && j < i)) continue;
            double v = ep.alpha * acc[g];
            if (ep.add) v += sig * ep.add[(long long)i * ep.ldo + j];
            if (ep.f32out) {
                ((float*)ep.out)[(long long)i * ep.ldo + j] = (float)v;
            } else {
                ((double*)ep.out)[(long long)i * ep.ldo + j] = v;
                if (ep.sym && j > i) ((double*)ep.out)[(long long)j * ep.ldo + i] = v;
            }
        }
    }
}

// ---- the small kernels -----------------------------------------------------------------------------------------------------------

__device__ __forceinline__ double pca_wave_sum(double v) {      // every lane receives the sum; a fixed order
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// column means in fp64: 32 columns x 8 row groups per workgroup, the groups added in order
__global__ __launch_bounds__(256) void pca_mean_kernel(const float* __restrict__ x, int n, int d, double* __restrict__ mean) {
    __shared__ double part[8][32];
    const int c = blockIdx.x * 32 + (threadIdx.x & 31), g = threadIdx.x >> 5;
    double sum = 0.0;
    if (c < d)
        for (int r = g; r < n; r += 8) sum += (double)x[(long long)r * d + c];
    part[g][threadIdx.x & 31] = sum;
    __syncthreads();
    if (g == 0 && c < d) {
        double t = part[0][threadIdx.x];
        for (int i = 1; i < 8; ++i) t += part[i][threadIdx.x];
        mean[c] = t / (double)n;
    }
}

// sigma = 2^-16 trace(C) / d
__global__ __launch_bounds__(256) void pca_sigma_kernel(const double* __restrict__ C, int d, double* __restrict__ sigma) {
    __shared__ double part[256];
    double sum = 0.0;
    for (int i = threadIdx.x; i < d; i += 256) sum += C[(long long)i * d + i];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < 256; ++i) t += part[i];
        *sigma = t / (double)d * (1.0 / 65536.0);
    }
}

// the start block: a counter-based hash of the element's index (splitmix64's finaliser), uniform in (-1, 1)
__global__ __launch_bounds__(256) void pca_start_kernel(double* __restrict__ q, long long count) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    unsigned long long z = ((unsigned long long)i + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    q[i] = 2.0 * ((double)(z >> 11) * (1.0 / 9007199254740992.0)) - 1.0;
}

enum { PCA_FLAG_CONVERGED = 0, PCA_FLAG_CHOL_FAILED = 1 };
constexpr int PCA_MAX_B = 384;     // k <= 256 -> b <= 256 + 128

// Cholesky G = U^T U of the symmetric b x b Gram matrix in one workgroup, left-looking: thread i owns column i of U.  A pivot that is
// not positive beyond rounding (the block's vectors are dependent to working precision) sets the failure flag and ends the kernel;
// the host reports it at its next read.
__global__ __launch_bounds__(PCA_MAX_B) void pca_chol_kernel(const double* __restrict__ G, double* U, int b, int* flags) {
    __shared__ double pivot;
    const int i = threadIdx.x;
    for (int j = 0; j < b; ++j) {
        double v = 0.0;
        if (i >= j && i < b) {
            v = G[(long long)j * b + i];
#pragma unroll 4
            for (int m = 0; m < j; ++m) v -= U[(long long)m * b + i] * U[(long long)m * b + j];
        }
        if (i == j) pivot = v;
        __syncthreads();
        const double p = pivot;
        if (!(p > 4e-14 * G[(long long)j * b + j])) {           // the same p in every thread: all leave together
            if (i == 0) flags[PCA_FLAG_CHOL_FAILED] = 1;
            return;
        }
        if (i >= j && i < b) U[(long long)j * b + i] = i == j ? sqrt(p) : v / sqrt(p);
        __syncthreads();
    }
}

// Z <- U^-T Z: forward substitution down each of the d columns of Zt [b,d], one thread per column (its earlier results are its own)
__global__ __launch_bounds__(64) void pca_solve_kernel(const double* __restrict__ U, double* Z, int b, int d) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= d) return;
    for (int i = 0; i < b; ++i) {
        double v = Z[(long long)i * d + j];
#pragma unroll 8
        for (int m = 0; m < i; ++m) v -= U[(long long)m * b + i] * Z[(long long)m * d + j];
        Z[(long long)i * d + j] = v / U[(long long)i * b + i];
    }
}

// Eigen-decomposition of the symmetric positive definite b x b matrix A in one workgroup by one-sided Jacobi on its rows: plane
// rotations make the rows of G A orthogonal; the same rotations applied to G = I leave G's rows the eigenvectors (A = A^T), and
// theta_i = a_i . g_i.  b / 2 disjoint row pairs per step (round-robin schedule), a wave per pair, a barrier per step.  The matrices
// live in global memory (b = 192: 295 KB each); a workgroup's waves share one L1, so the barrier orders their accesses.  Out: the
// eigenvalues in descending order and the eigenvectors as rows in that order.  Ends when a sweep rotates nothing, or after
// PCA_JACOBI_SWEEPS -- the caller's residual test judges the result either way.
constexpr int PCA_JACOBI_SWEEPS = 30;
__global__ __launch_bounds__(1024) void pca_jacobi_kernel(double* A, double* G, int b, double* vt, double* theta) {
    __shared__ double th[PCA_MAX_B];
    __shared__ int rank[PCA_MAX_B];
    __shared__ int rotated;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int e = tid; e < b * b; e += 1024) G[e] = e / b == e % b ? 1.0 : 0.0;
    const int m = b + (b & 1);
    const double tol = sqrt((double)(b < 16 ? 16 : b)) * 2.220446049250313e-16;
    for (int sweep = 0; sweep < PCA_JACOBI_SWEEPS; ++sweep) {
        if (tid == 0) rotated = 0;
        __syncthreads();
        for (int step = 0; step < m - 1; ++step) {
            for (int p = wave; p < m / 2; p += 16) {
                int i = p == 0 ? m - 1 : (step + p) % (m - 1);
                int j = p == 0 ? step : (step - p + m - 1) % (m - 1);
                if (i >= b || j >= b) continue;                 // the dummy of an odd b
                if (i > j) { const int t = i; i = j; j = t; }
                double* ai = A + (long long)i * b;
                double* aj = A + (long long)j * b;
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int c = lane; c < b; c += 64) {
                    const double u = ai[c], w = aj[c];
                    alpha += u * u;
                    beta += w * w;
                    gamma += u * w;
                }
                alpha = pca_wave_sum(alpha);
                beta = pca_wave_sum(beta);
                gamma = pca_wave_sum(gamma);
                if (!(fabs(gamma) > tol * sqrt(alpha * beta))) continue;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                double* gi = G + (long long)i * b;
                double* gj = G + (long long)j * b;
                for (int c = lane; c < b; c += 64) {
                    const double u = ai[c], w = aj[c];
                    ai[c] = cs * u - sn * w;
                    aj[c] = sn * u + cs * w;
                    const double gu = gi[c], gw = gj[c];
                    gi[c] = cs * gu - sn * gw;
                    gj[c] = sn * gu + cs * gw;
                }
                if (lane == 0) rotated = 1;
            }
            __syncthreads();
        }
        const int again = rotated;
        __syncthreads();
        if (!again) break;
    }
    for (int i = wave; i < b; i += 16) {
        double s = 0.0;
        for (int c = lane; c < b; c += 64) s += A[(long long)i * b + c] * G[(long long)i * b + c];
        s = pca_wave_sum(s);
        if (lane == 0) th[i] = s;
    }
    __syncthreads();
    for (int i = tid; i < b; i += 1024) {                       // descending, equal values in index order
        int rk = 0;
        for (int j = 0; j < b; ++j) rk += (th[j] > th[i] || (th[j] == th[i] && j < i)) ? 1 : 0;
        rank[i] = rk;
        theta[rk] = th[i];
    }
    __syncthreads();
    for (int i = wave; i < b; i += 16)
        for (int c = lane; c < b; c += 64) vt[(long long)rank[i] * b + c] = G[(long long)i * b + c];
}

// The first k Ritz pairs, one workgroup: theta_i = the Rayleigh quotient of row i of Q with Z = (C + sigma) Q -- computed from the
// rotated vectors themselves, so that a small eigenvalue keeps its relative accuracy next to a large one -- replaces the Jacobi
// value, and |Z_i - theta_i Q_i| is held against tol * lambda_1.
__global__ __launch_bounds__(1024) void pca_check_kernel(const double* __restrict__ Q, const double* __restrict__ Z, double* theta,
                                                         const double* __restrict__ sigma, int k, int d, double tol, int* flags) {
    __shared__ double res[256];
    __shared__ double first;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = wave; i < k; i += 16) {
        double zq = 0.0, qq = 0.0;
        for (int c = lane; c < d; c += 64) {
            const double q = Q[(long long)i * d + c];
            zq += Z[(long long)i * d + c] * q;
            qq += q * q;
        }
        const double th = pca_wave_sum(zq) / pca_wave_sum(qq);
        double s = 0.0;
        for (int c = lane; c < d; c += 64) {
            const double e = Z[(long long)i * d + c] - th * Q[(long long)i * d + c];
            s += e * e;
        }
        s = pca_wave_sum(s);
        if (lane == 0) {
            theta[i] = th;
            res[i] = sqrt(s);
            if (i == 0) first = th;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double bound = tol * (first - *sigma);
        int ok = 1;
        for (int i = 0; i < k; ++i) ok = (ok && res[i] <= bound) ? 1 : 0;      // a NaN is not converged
        flags[PCA_FLAG_CONVERGED] = ok;
    }
}

// components[i] = +- Q[i] with the entry of largest magnitude positive (the first one on ties), explained_variance[i] = theta_i - sigma
__global__ __launch_bounds__(256) void pca_finish_kernel(const double* __restrict__ Q, const double* __restrict__ theta,
                                                         const double* __restrict__ sigma, int d, double* __restrict__ components,
                                                         double* __restrict__ ev, int* __restrict__ info, int iterations, int converged) {
    __shared__ double bv[256];
    __shared__ int bi[256];
    const int i = blockIdx.x, tid = threadIdx.x;
    const double* q = Q + (long long)i * d;
    double best = -1.0;
    int at = 0;
    for (int c = tid; c < d; c += 256) {
        const double a = fabs(q[c]);
        if (a > best) { best = a; at = c; }
    }
    bv[tid] = best;
    bi[tid] = at;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if (tid < h && (bv[tid + h] > bv[tid] || (bv[tid + h] == bv[tid] && bi[tid + h] < bi[tid]))) {
            bv[tid] = bv[tid + h];
            bi[tid] = bi[tid + h];
        }
        __syncthreads();
    }
    const double sign = q[bi[0]] < 0.0 ? -1.0 : 1.0;
    for (int c = tid; c < d; c += 256) components[(long long)i * d + c] = sign * q[c];
    if (tid == 0) {
        ev[i] = theta[i] - *sigma;
        if (i == 0) { info[0] = iterations; info[1] = converged; }
    }
}

size_t pca_up16(size_t b) { return (b + 15) & ~(size_t)15; }

int pca_gemm(const PcaOperand& A, const PcaOperand& B, int M, int N, int K, const PcaEpilogue& ep, const char* what, hipStream_t s) {
    const dim3 grid((M + PCA_TM - 1) / PCA_TM, (N + PCA_TN - 1) / PCA_TN);
    HSEFR_LAUNCH(pca_gemm_kernel, grid, dim3(256), 0, s, A, B, M, K, ep);
    return launch_status(what);
}

PcaOperand rows_of(const double* p, int rows, int ld) { return PcaOperand{p, ld, 1, rows, nullptr}; }        // (r, k) = p[r][k]
PcaOperand cols_of(const double* p, int cols, int ld) { return PcaOperand{p, 1, ld, cols, nullptr}; }        // (r, k) = p[k][r]
PcaEpilogue f64_out(double* out, int ld, int ncols, int sym) { return PcaEpilogue{out, ld, 0, ncols, sym, 1.0, nullptr, nullptr}; }

}  // namespace

int launch_pca_fit(const float* x, int n, int d, int k, int max_iter, double* mean, double* components, double* explained_variance,
                   int* info, hipStream_t s) {
    HSEFR_REQUIRE(d > 0 && d % 8 == 0, HSEFR_ERR_UNSUPPORTED, "pca_fit: d=%d must be a multiple of 8", d);
    HSEFR_REQUIRE(n >= 2, HSEFR_ERR_INVALID, "pca_fit: n=%d rows, at least 2 are needed", n);
    const int cap = n - 1 < d ? n - 1 : d;
    HSEFR_REQUIRE(k >= 1 && k <= cap && k <= 256, HSEFR_ERR_INVALID, "pca_fit: k=%d must be in 1..min(n - 1, d, 256) with n=%d d=%d", k, n, d);
    HSEFR_REQUIRE(max_iter >= 1, HSEFR_ERR_INVALID, "pca_fit: max_iter=%d must be at least 1", max_iter);
    // the block: k plus max(16, k / 2) oversampling vectors, in sixteens; never more than the covariance has directions
    int b = (k + (k / 2 > 16 ? k / 2 : 16) + 15) / 16 * 16;
    if (b > cap) b = cap;
    const size_t bd = pca_up16((size_t)b * d * 8), bb = pca_up16((size_t)b * b * 8);
    const size_t bytes = pca_up16((size_t)d * d * 8) + 4 * bd + 5 * bb + pca_up16((size_t)b * 8) + 16 + 16;
    char* ws = nullptr;
    if (hipMallocAsync((void**)&ws, bytes, s) != hipSuccess || !ws) {
        (void)hipGetLastError();
        set_error("pca_fit: no stream-ordered workspace (%zu bytes: the %d x %d fp64 covariance and four %d x %d blocks) for n=%d d=%d k=%d",
                  bytes, d, d, b, d, n, d, k);
        return HSEFR_ERR_NOMEM;
    }
    char* p = ws;
    auto take = [&p](size_t nbytes) { char* q = p; p += nbytes; return q; };
    double* C = (double*)take(pca_up16((size_t)d * d * 8));
    double* Q = (double*)take(bd);
    double* Z = (double*)take(bd);
    double* S1 = (double*)take(bd);
    double* S2 = (double*)take(bd);
    double* Gram = (double*)take(bb);
    double* U = (double*)take(bb);
    double* T = (double*)take(bb);
    double* Gw = (double*)take(bb);
    double* Vt = (double*)take(bb);
    double* theta = (double*)take(pca_up16((size_t)b * 8));
    double* sigma = (double*)take(16);
    int* flags = (int*)take(16);

    int rc = HSEFR_OK;
    hipError_t e = hipMemsetAsync(flags, 0, 16, s);
    // Z <- orthonormal rows spanning Z's: CholeskyQR, `passes` times (the second pass brings |Q Q^T - I| down to rounding)
    const auto orthonormalise = [&](double* Zt, int passes) {
        for (int pass = 0; pass < passes && rc == HSEFR_OK; ++pass) {
            rc = pca_gemm(rows_of(Zt, b, d), rows_of(Zt, b, d), b, b, d, f64_out(Gram, b, b, 1), "pca_fit (Gram matrix)", s);
            if (rc != HSEFR_OK) break;
            HSEFR_LAUNCH(pca_chol_kernel, dim3(1), dim3(PCA_MAX_B), 0, s, Gram, U, b, flags);
            HSEFR_LAUNCH(pca_solve_kernel, dim3((d + 63) / 64), dim3(64), 0, s, U, Zt, b, d);
            rc = launch_status("pca_fit (CholeskyQR)");
        }
    };
    if (e == hipSuccess) {
        HSEFR_LAUNCH(pca_mean_kernel, dim3((d + 31) / 32), dim3(256), 0, s, x, n, d, mean);
        rc = launch_status("pca_fit (column means)");
    }
    if (rc == HSEFR_OK && e == hipSuccess) {
        const PcaOperand xc{x, 1, d, d, mean};                 // (feature r, sample k) = x[k][r] - mean[r]
        PcaEpilogue ep = f64_out(C, d, d, 1);
        ep.alpha = 1.0 / (double)(n - 1);
        rc = pca_gemm(xc, xc, d, d, n, ep, "pca_fit (covariance)", s);
    }
    if (rc == HSEFR_OK && e == hipSuccess) {
        HSEFR_LAUNCH(pca_sigma_kernel, dim3(1), dim3(256), 0, s, C, d, sigma);
        const long long count = (long long)b * d;
        HSEFR_LAUNCH(pca_start_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, Q, count);
        rc = launch_status("pca_fit (start block)");
        orthonormalise(Q, 2);
    }
    int it = 0, converged = 0, chol_failed = 0;
    const int every = 8;                                       // Rayleigh-Ritz does not change the span: only at convergence checks
    while (rc == HSEFR_OK && e == hipSuccess) {
        PcaEpilogue ep = f64_out(Z, d, d, 0);                  // Z = Q C + sigma Q  (C is symmetric: (j, k) = C[j][k])
        ep.sigma = sigma;
        ep.add = Q;
        rc = pca_gemm(rows_of(Q, b, d), rows_of(C, d, d), b, d, d, ep, "pca_fit (C Q)", s);
        if (rc != HSEFR_OK) break;
        ++it;
        // with b == d the block spans the whole space and the first Rayleigh-Ritz step is the eigen-decomposition itself
        if (it % every == 0 || it >= max_iter || (it == 1 && b == d)) {
            rc = pca_gemm(rows_of(Z, b, d), rows_of(Q, b, d), b, b, d, f64_out(T, b, b, 1), "pca_fit (Rayleigh-Ritz matrix)", s);
            if (rc != HSEFR_OK) break;
            HSEFR_LAUNCH(pca_jacobi_kernel, dim3(1), dim3(1024), 0, s, T, Gw, b, Vt, theta);
            rc = launch_status("pca_fit (Jacobi)");
            if (rc == HSEFR_OK) rc = pca_gemm(rows_of(Vt, b, b), cols_of(Q, d, d), b, d, b, f64_out(S1, d, d, 0), "pca_fit (rotation)", s);
            if (rc == HSEFR_OK) {                               // Z of the rotated vectors, afresh: a rotated Z would carry lambda_1's rounding into every row
                PcaEpilogue e2 = f64_out(S2, d, d, 0);
                e2.sigma = sigma;
                e2.add = S1;
                rc = pca_gemm(rows_of(S1, b, d), rows_of(C, d, d), b, d, d, e2, "pca_fit (C Q)", s);
            }
            if (rc != HSEFR_OK) break;
            { double* t = Q; Q = S1; S1 = t; t = Z; Z = S2; S2 = t; }
            HSEFR_LAUNCH(pca_check_kernel, dim3(1), dim3(1024), 0, s, Q, Z, theta, sigma, k, d, 1e-10, flags);
            rc = launch_status("pca_fit (residuals)");
            if (rc != HSEFR_OK) break;
            int host_flags[2] = {0, 0};
            e = hipMemcpyAsync(host_flags, flags, sizeof(host_flags), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) break;
            converged = host_flags[PCA_FLAG_CONVERGED];
            chol_failed = host_flags[PCA_FLAG_CHOL_FAILED];
            if (converged || chol_failed || it >= max_iter) break;
        }
        const bool check_next = (it + 1) % every == 0 || it + 1 >= max_iter;
        orthonormalise(Z, check_next ? 2 : 1);
        { double* t = Q; Q = Z; Z = t; }
    }
    if (rc == HSEFR_OK && e == hipSuccess && chol_failed) {
        set_error("pca_fit: a Cholesky pivot of the %d x %d Gram matrix was not positive after %d iterations: the rows have no variance, "
                  "or hold values that are not finite (n=%d d=%d k=%d)", b, b, it, n, d, k);
        rc = HSEFR_ERR_INVALID;
    }
    if (rc == HSEFR_OK && e == hipSuccess) {
        HSEFR_LAUNCH(pca_finish_kernel, dim3(k), dim3(256), 0, s, Q, theta, sigma, d, components, explained_variance, info, it, converged);
        rc = launch_status("pca_fit (components)");
    }
    if (rc == HSEFR_OK && e != hipSuccess) {
        set_error("pca_fit: clearing or reading the convergence flags failed: %s", hipGetErrorString(e));
        rc = HSEFR_ERR_HIP;
    }
    (void)hipFreeAsync(ws, s);
    return rc;
}

int launch_pca_transform(const float* x, int n, int d, int k, const double* mean, const double* components, float* z, int ldz,
                         hipStream_t s) {
    HSEFR_REQUIRE(d > 0 && d % 8 == 0, HSEFR_ERR_UNSUPPORTED, "pca_transform: d=%d must be a multiple of 8", d);
    HSEFR_REQUIRE(n >= 0, HSEFR_ERR_INVALID, "pca_transform: n=%d", n);
    HSEFR_REQUIRE(k >= 1 && k <= d && k <= 256, HSEFR_ERR_INVALID, "pca_transform: k=%d must be in 1..min(d, 256) with d=%d", k, d);
    HSEFR_REQUIRE(ldz >= k && ldz % 8 == 0, HSEFR_ERR_INVALID, "pca_transform: ldz=%d must be a multiple of 8 and at least k=%d", ldz, k);
    if (n == 0) return HSEFR_OK;
    const PcaOperand xc{x, d, 1, n, mean};                     // (row r, feature k) = x[r][k] - mean[k]
    const PcaEpilogue ep{z, ldz, 1, ldz, 0, 1.0, nullptr, nullptr};
    return pca_gemm(xc, rows_of(components, k, d), n, ldz, d, ep, "pca_transform", s);
}

}  // namespace hsefr
