// sklearn.svm.SVC() (facerec_test.py:269-288 'svm') on the device, at the optimum of its objective: hsefr_rbf_svm_gamma_scale /
// hsefr_rbf_svm_fit / hsefr_rbf_svm_decision / hsefr_rbf_svm_predict.
//
// libsvm's C-SVC with the RBF kernel, one-vs-one: for every pair of classes (i, j), i < j, class i is +1 and the dual
//     min 1/2 a^T Q a - e^T a ,  0 <= a <= C ,  y^T a = 0 ,  Q_ab = y_a y_b exp(-gamma |x_a - x_b|^2)
// is solved over the rows of the two classes.  For distinct rows Q is positive definite: the minimiser is unique.  Q is libsvm's: its
// solver holds every kernel value as a float (Qfloat), so SVC's optimum is that of the ROUNDED matrix -- about 1e-8 in decision values
// from the unrounded one's.  The Gram matrix here is computed in fp64, rounded once to fp32 and then used as fp64 throughout; the
// kernel values of the probes are not rounded (libsvm's predict does not round them either).
//   - The rows are grouped by class once (a stable counting sort on the device: `perm`), so a pair's rows are two runs of one fp64 Gram
//     matrix, built by the product kernel of csrc/linear_svm.hip with its RBF epilogue (csrc/svm_gemm.h).
//   - Every pair is an independent SMO with libsvm's second-order working set selection and its clipping, from a = 0, to
//     m(a) - M(a) <= tol.  The host sorts the pairs by their number of rows: those over 64 rows take a 256-thread workgroup each, the
//     largest first; the others a wave each.  The state (a, the gradient) lives in LDS, beyond 1024 rows in a workspace.
//   - rho follows libsvm's rule: the mean of y G over the free variables, without one the midpoint of the bounds.
//   - Prediction never forms the pair decisions of all probes: per tile of at most 1024 probes one kernel matrix [gallery, probes] and
//     one pass over dual_coef, a wave per (class i, 32 opponents j, 64 probes); a decision value is computed in ONE place (the rows of i
//     in order, then the rows of j, then - rho), so both classes see the same sign.  Votes are integer atomics (their order changes no sum).
// Every floating-point sum has a fixed shape: two fits give equal bits.
#include "common.h"
#include "svm_gemm.h"

#include <float.h>
#include <math.h>

#include <vector>

namespace hsefr {
namespace {

// the limits of the entry points: the LFW half split (4582 x 1024, 1680 classes: 1 410 360 pairs) is inside
constexpr int RBF_MAX_N = 1 << 14, RBF_MAX_D = 1 << 14, RBF_MAX_CLASSES = 1 << 12;
constexpr long long RBF_MAX_DECISIONS = 1ll << 27;           // nq * P of hsefr_rbf_svm_decision: 1 GiB of fp64
constexpr int RBF_WAVE_ROWS = 64;                            // a pair of up to this many rows is solved by one wave
constexpr int RBF_LDS_ROWS = 1024;                           // a workgroup keeps a pair of up to this many rows in LDS
constexpr int RBF_WAVE_PAIRS = 8;                            // pairs a one-wave workgroup solves one after another
constexpr int RBF_TILE_Q = 1024;                             // probes per kernel matrix of predict / decision
constexpr int RBF_OPPONENTS = 32;                            // opponents j of one class i per wave of the vote kernel
enum { RBF_FLAG_BAD_LABEL = 0, RBF_FLAG_EMPTY_CLASS = 1, RBF_FLAGS = 4 };

// ---- gamma = 'scale' ------------------------------------------------------------------------------------------------------------------

__device__ double rbf_block_sum(double v, double* part /* [4], shared */) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return (part[0] + part[1]) + (part[2] + part[3]);
}

// 256 workgroups whatever the size: partial[b] = the sum over elements b * 256 + tid + 65536 k of x (mean == null) or (x - mean)^2
__global__ __launch_bounds__(256) void rbf_moment_kernel(const float* __restrict__ x, int n, int d, int d_used, const double* mean,
                                                         double* partial) {
    __shared__ double part[4];
    const long long total = (long long)n * d_used;
    const double mu = mean ? mean[0] : 0.0;
    double sum = 0.0;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += 65536) {
        const double v = (double)x[(e / d_used) * d + e % d_used];
        sum += mean ? (v - mu) * (v - mu) : v;
    }
    sum = rbf_block_sum(sum, part);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}
// one workgroup: last == 0 writes the mean, last == 1 gamma = 1 / (d_used * variance), 1 where the variance is 0
__global__ __launch_bounds__(256) void rbf_moment_finish_kernel(const double* partial, double total, int d_used, int last, double* out) {
    __shared__ double part[4];
    const double sum = rbf_block_sum(partial[threadIdx.x], part);
    if (threadIdx.x != 0) return;
    const double v = sum / total;
    out[0] = !last ? v : (v > 0.0 ? 1.0 / ((double)d_used * v) : 1.0);
}

// ---- rows grouped by class --------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void rbf_count_kernel(const int* __restrict__ labels, int n, int K, int* counts, int* flags) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    const int c = labels[a];
    if (c < 0 || c >= K) flags[RBF_FLAG_BAD_LABEL] = 1;      // every writer stores the same 1
    else atomicAdd(&counts[c], 1);
}
// start [K + 1]: the exclusive prefix sums of counts, one workgroup; an empty class raises its flag
__global__ __launch_bounds__(256) void rbf_scan_kernel(const int* __restrict__ counts, int K, int* start, int* flags) {
    __shared__ int chunk[256];
    const int tid = threadIdx.x, per = (K + 255) / 256, c0 = tid * per;
    int sum = 0;
    for (int c = c0; c < c0 + per && c < K; ++c) {
        sum += counts[c];
        if (counts[c] == 0) flags[RBF_FLAG_EMPTY_CLASS] = 1;
    }
    chunk[tid] = sum;
    __syncthreads();
    int at = 0;
    for (int t = 0; t < tid; ++t) at += chunk[t];
    for (int c = c0; c < c0 + per && c < K; ++c) {
        start[c] = at;
        at += counts[c];
    }
    if (tid == 255) start[K] = at;
}
// perm [n]: the caller's row of each grouped position -- class by class, inside a class in the caller's order
__global__ __launch_bounds__(256) void rbf_rank_kernel(const int* __restrict__ labels, int n, const int* __restrict__ start, int* perm) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    const int c = labels[a];
    int before = 0;
    for (int b = 0; b < a; ++b) before += labels[b] == c ? 1 : 0;
    perm[start[c] + before] = a;
}
// a wave per row g: norm[g] = |x[perm[g]]|^2 in fp64, and the row copied to xs[g] (xs, perm may be null: the rows as they are)
__global__ __launch_bounds__(64) void rbf_rows_kernel(const float* __restrict__ x, int n, int d, const int* __restrict__ perm, float* xs,
                                                      double* norm) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const float* row = x + (long long)(perm ? perm[g] : g) * d;
    double sum = 0.0;
    for (int c = lane; c < d; c += 64) {
        const float v = row[c];
        if (xs) xs[(long long)g * d + c] = v;
        sum += (double)v * (double)v;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) norm[g] = sum;
}
// dcs[r][g] = dual_coef[r][perm[g]]
__global__ __launch_bounds__(256) void rbf_group_coef_kernel(const double* __restrict__ dual_coef, int rows, int n, const int* __restrict__ perm,
                                                            double* dcs) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)rows * n) return;
    dcs[e] = dual_coef[(e / n) * n + perm[e % n]];
}

// ---- one pair's SMO ------------------------------------------------------------------------------------------------------------------------

struct RbfFit {
    const double* gram;          // [n, n] over the grouped rows
    int n, K;
    const int* start;            // [K + 1]
    const int* perm;             // [n]
    const int2* pairs;           // sorted by size, the largest first
    long long first, count;      // this launch's pairs
    const long long* scratch_at; // for the pairs over RBF_LDS_ROWS rows (they come first): where their 2 m doubles start
    double* scratch;
    double C, tol;
    int max_iter;
    double* dual_coef;           // [(K - 1), n], the caller's row order
    double* rho;                 // [K (K - 1) / 2], libsvm's pair order
    int* info;                   // [0] the most iterations, [2] the pairs that reached max_iter
};

// (v, idx): the largest v, the lowest idx among equals; w: the largest w -- in every thread of the T-thread workgroup
template <int T>
__device__ __forceinline__ void rbf_arg_reduce(double& v, int& idx, double& w, double* sv, int* si, double* sw) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double ov = __shfl_xor(v, o), ow = __shfl_xor(w, o);
        const int oi = __shfl_xor(idx, o);
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
        w = ow > w ? ow : w;
    }
    if (T > 64) {
        __syncthreads();                                      // the previous call's values have been read
        if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; si[threadIdx.x >> 6] = idx; sw[threadIdx.x >> 6] = w; }
        __syncthreads();
        v = sv[0]; idx = si[0]; w = sw[0];
#pragma unroll
        for (int k = 1; k < T / 64; ++k) {
            if (sv[k] > v || (sv[k] == v && si[k] < idx)) { v = sv[k]; idx = si[k]; }
            w = sw[k] > w ? sw[k] : w;
        }
    }
}

template <int T, int CAP, int PER>
__global__ __launch_bounds__(T) void rbf_smo_kernel(RbfFit a) {
    __shared__ double s_alpha[CAP], s_grad[CAP];
    __shared__ double sv[4], sw[4];
    __shared__ int si[4];
    const int tid = threadIdx.x;
    for (int rep = 0; rep < PER; ++rep) {
        const long long slot = (long long)blockIdx.x * PER + rep;
        if (slot >= a.count) break;                           // the same in every thread
        const long long pi = a.first + slot;
        const int ci = a.pairs[pi].x, cj = a.pairs[pi].y;
        const int s_i = a.start[ci], ni = a.start[ci + 1] - s_i, s_j = a.start[cj], m = ni + a.start[cj + 1] - s_j;
        double* alpha = m <= CAP ? s_alpha : a.scratch + a.scratch_at[pi];
        double* grad = m <= CAP ? s_grad : alpha + m;
        const double C = a.C;
        __syncthreads();                                      // the previous pair's state has been read
        for (int t = tid; t < m; t += T) { alpha[t] = 0.0; grad[t] = -1.0; }
        __syncthreads();
        int iter = 0, capped = 0;
        for (;;) {
            // i = arg max over I_up of -y G; Gmax2 = max over I_low of y G
            double gmax = -INFINITY, gmax2 = -INFINITY;
            int i = -1;
            for (int t = tid; t < m; t += T) {
                const double al = alpha[t], yg = t < ni ? grad[t] : -grad[t];
                const bool up = t < ni ? al < C : al > 0.0, low = t < ni ? al > 0.0 : al < C;
                if (up && -yg > gmax) { gmax = -yg; i = t; }
                if (low && yg > gmax2) gmax2 = yg;
            }
            rbf_arg_reduce<T>(gmax, i, gmax2, sv, si, sw);
            if (gmax + gmax2 <= a.tol) break;
            if (iter >= a.max_iter || i < 0) { capped = 1; break; }
            const double* Ki = a.gram + (long long)(i < ni ? s_i + i : s_j + i - ni) * a.n;
            // j = arg min over I_low with -y G < Gmax of -(Gmax + y G)^2 / (K_ii + K_tt - 2 K_it)
            double best = -INFINITY, unused = 0.0;
            int j = -1;
            for (int t = tid; t < m; t += T) {
                const double al = alpha[t], yg = t < ni ? grad[t] : -grad[t];
                const bool low = t < ni ? al > 0.0 : al < C;
                const double diff = gmax + yg;
                if (low && diff > 0.0) {
                    double quad = 2.0 - 2.0 * Ki[t < ni ? s_i + t : s_j + t - ni];
                    if (!(quad > 0.0)) quad = 1e-12;
                    const double gain = diff * diff / quad;
                    if (gain > best) { best = gain; j = t; }
                }
            }
            rbf_arg_reduce<T>(best, j, unused, sv, si, sw);
            if (j < 0) { capped = 1; break; }
            const double* Kj = a.gram + (long long)(j < ni ? s_i + j : s_j + j - ni) * a.n;
            const double yi = i < ni ? 1.0 : -1.0, yj = j < ni ? 1.0 : -1.0;
            const double ai = alpha[i], aj = alpha[j], gi = grad[i], gj = grad[j];
            double quad = 2.0 - 2.0 * Ki[j < ni ? s_i + j : s_j + j - ni];
            if (!(quad > 0.0)) quad = 1e-12;
            double bi, bj;                                    // libsvm's step and clipping, C the same for both
            if (yi != yj) {
                const double delta = (-gi - gj) / quad, diff = ai - aj;
                bi = ai + delta; bj = aj + delta;
                if (diff > 0.0) { if (bj < 0.0) { bj = 0.0; bi = diff; } }
                else if (bi < 0.0) { bi = 0.0; bj = -diff; }
                if (diff > 0.0) { if (bi > C) { bi = C; bj = C - diff; } }
                else if (bj > C) { bj = C; bi = C + diff; }
            } else {
                const double delta = (gi - gj) / quad, sum = ai + aj;
                bi = ai - delta; bj = aj + delta;
                if (sum > C) { if (bi > C) { bi = C; bj = sum - C; } }
                else if (bj < 0.0) { bj = 0.0; bi = sum; }
                if (sum > C) { if (bj > C) { bj = C; bi = sum - C; } }
                else if (bi < 0.0) { bi = 0.0; bj = sum; }
            }
            const double di = yi * (bi - ai), dj = yj * (bj - aj);
            __syncthreads();                                  // every thread has read alpha and the gradient of i and j
            for (int t = tid; t < m; t += T) {
                const int g = t < ni ? s_i + t : s_j + t - ni;
                const double q = Ki[g] * di + Kj[g] * dj;
                grad[t] += t < ni ? q : -q;
            }
            if (tid == 0) { alpha[i] = bi; alpha[j] = bj; }
            __syncthreads();
            ++iter;
        }
        // rho: the mean of y G over the free variables, else the midpoint of the bounds (-ub and lb as maxima)
        double nub = -INFINITY, lb = -INFINITY, free_sum = 0.0;
        int free_count = 0;
        for (int t = tid; t < m; t += T) {
            const double al = alpha[t], yg = t < ni ? grad[t] : -grad[t];
            const bool pos = t < ni;
            if (al >= C) { if (pos) lb = yg > lb ? yg : lb; else nub = -yg > nub ? -yg : nub; }
            else if (al <= 0.0) { if (pos) nub = -yg > nub ? -yg : nub; else lb = yg > lb ? yg : lb; }
            else { ++free_count; free_sum += yg; }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            free_sum += __shfl_xor(free_sum, o);
            free_count += __shfl_xor(free_count, o);
        }
        int none = 0;
        rbf_arg_reduce<T>(nub, none, lb, sv, si, sw);
        if (T > 64) {
            __shared__ double fs[4];
            __shared__ int fc[4];
            __syncthreads();
            if ((tid & 63) == 0) { fs[tid >> 6] = free_sum; fc[tid >> 6] = free_count; }
            __syncthreads();
            free_sum = (fs[0] + fs[1]) + (fs[2] + fs[3]);
            free_count = fc[0] + fc[1] + fc[2] + fc[3];
        }
        for (int t = tid; t < m; t += T) {
            const int g = t < ni ? s_i + t : s_j + t - ni, row = t < ni ? cj - 1 : ci;
            a.dual_coef[(long long)row * a.n + a.perm[g]] = t < ni ? alpha[t] : -alpha[t];
        }
        if (tid == 0) {
            a.rho[(long long)ci * a.K - (long long)ci * (ci + 1) / 2 + (cj - ci - 1)] = free_count > 0 ? free_sum / free_count : (lb - nub) / 2.0;
            atomicMax(&a.info[0], iter);
            if (capped) atomicAdd(&a.info[2], 1);
        }
    }
}

__global__ void rbf_info_kernel(int* info) { info[1] = info[2] == 0 ? 1 : 0; }

// ---- decisions and votes -----------------------------------------------------------------------------------------------------------------

struct RbfVote {
    const double* kqt;           // [n, ldq]: the kernel of grouped gallery row g and probe q0 + q
    const double* dcs;           // [(K - 1), n]: dual_coef over the grouped rows
    const double* rho;
    const int* start;
    const int2* tasks;           // (class i, first opponent j)
    int n, K, ldq, nq, q0;
    long long P;
    int* votes_t;                // [K, ldq], or null
    double* out;                 // [., P] decisions, or null
};

// a wave: class i against opponents j0 .. j0 + 31 for 64 probes.  The value of a pair is formed here and nowhere else.
__global__ __launch_bounds__(64) void rbf_vote_kernel(RbfVote a) {
    const int ci = a.tasks[blockIdx.x].x, j0 = a.tasks[blockIdx.x].y;
    const int q = blockIdx.y * 64 + threadIdx.x, ql = q < a.nq ? q : a.nq - 1;
    const int s_i = a.start[ci], e_i = a.start[ci + 1];
    const double* own = a.dcs + (long long)ci * a.n;
    const long long p0 = (long long)ci * a.K - (long long)ci * (ci + 1) / 2 - ci - 1;
    int wins = 0;
    for (int cj = j0; cj < j0 + RBF_OPPONENTS && cj < a.K; ++cj) {
        const double* other = a.dcs + (long long)(cj - 1) * a.n;
        double acc = 0.0;
        for (int g = s_i; g < e_i; ++g) acc = fma(other[g], a.kqt[(long long)g * a.ldq + ql], acc);
        for (int g = a.start[cj]; g < a.start[cj + 1]; ++g) acc = fma(own[g], a.kqt[(long long)g * a.ldq + ql], acc);
        const double dec = acc - a.rho[p0 + cj];
        if (q >= a.nq) continue;
        if (a.out) a.out[(long long)(a.q0 + q) * a.P + p0 + cj] = dec;
        if (a.votes_t) {
            if (dec > 0.0) ++wins;
            else atomicAdd(&a.votes_t[(long long)cj * a.ldq + q], 1);
        }
    }
    if (a.votes_t && q < a.nq && wins) atomicAdd(&a.votes_t[(long long)ci * a.ldq + q], wins);
}
// a thread per probe: the first class with the most votes
__global__ __launch_bounds__(64) void rbf_label_kernel(const int* __restrict__ votes_t, int K, int ldq, int nq, int q0, int* pred, int* votes) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= nq) return;
    int best = -1, at = 0;
    for (int c = 0; c < K; ++c) {
        const int v = votes_t[(long long)c * ldq + q];
        if (v > best) { best = v; at = c; }
        if (votes) votes[(long long)(q0 + q) * K + c] = v;
    }
    pred[q0 + q] = at;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------------

size_t rbf_up(size_t b) { return (b + 255) & ~(size_t)255; }

struct RbfModel {                // the rows grouped by class, on the device and (start) on the host
    char* ws = nullptr;
    char* free_bytes = nullptr;  // the caller's share of the workspace
    int *counts = nullptr, *start = nullptr, *flags = nullptr, *perm = nullptr;
    float* xs = nullptr;
    double* norm = nullptr;
    std::vector<int> h_start;
};

// validates the labels, groups the rows and copies them: after it `stream` is synchronised and m.h_start holds the class offsets
int rbf_group_rows(const char* who, const float* x, int n, int d, const int* labels, int K, size_t extra, RbfModel& m, hipStream_t s) {
    const size_t ints = rbf_up((size_t)(2 * K + 1 + RBF_FLAGS) * 4), perm_b = rbf_up((size_t)n * 4), xs_b = rbf_up((size_t)n * d * 4),
                 norm_b = rbf_up((size_t)n * 8), total = ints + perm_b + xs_b + norm_b + extra;
    if (hipMallocAsync((void**)&m.ws, total, s) != hipSuccess || !m.ws) {
        (void)hipGetLastError();
        m.ws = nullptr;
        set_error("%s: no stream-ordered workspace (%zu bytes) for n=%d d=%d n_classes=%d", who, total, n, d, K);
        return HSEFR_ERR_NOMEM;
    }
    m.counts = (int*)m.ws; m.start = m.counts + K; m.flags = m.start + K + 1;
    m.perm = (int*)(m.ws + ints); m.xs = (float*)(m.ws + ints + perm_b); m.norm = (double*)(m.ws + ints + perm_b + xs_b);
    m.free_bytes = m.ws + ints + perm_b + xs_b + norm_b;
    hipError_t e = hipMemsetAsync(m.ws, 0, ints, s);
    if (e != hipSuccess) { set_error("%s: clearing the class counts failed: %s", who, hipGetErrorString(e)); return HSEFR_ERR_HIP; }
    HSEFR_LAUNCH(rbf_count_kernel, dim3((n + 255) / 256), dim3(256), 0, s, labels, n, K, m.counts, m.flags);
    HSEFR_LAUNCH(rbf_scan_kernel, dim3(1), dim3(256), 0, s, (const int*)m.counts, K, m.start, m.flags);
    int rc = launch_status(who);
    if (rc != HSEFR_OK) return rc;
    std::vector<int> host(K + 1 + RBF_FLAGS);
    e = hipMemcpyAsync(host.data(), m.start, host.size() * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { set_error("%s: reading the class sizes failed: %s", who, hipGetErrorString(e)); return HSEFR_ERR_HIP; }
    if (host[K + 1 + RBF_FLAG_BAD_LABEL]) {
        set_error("%s: a label code is outside 0..%d (n=%d)", who, K - 1, n);
        return HSEFR_ERR_INVALID;
    }
    if (host[K + 1 + RBF_FLAG_EMPTY_CLASS]) {
        set_error("%s: a class of 0..%d has no row (n=%d)", who, K - 1, n);
        return HSEFR_ERR_INVALID;
    }
    m.h_start.assign(host.begin(), host.begin() + K + 1);
    HSEFR_LAUNCH(rbf_rank_kernel, dim3((n + 255) / 256), dim3(256), 0, s, labels, n, (const int*)m.start, m.perm);
    HSEFR_LAUNCH(rbf_rows_kernel, dim3(n), dim3(64), 0, s, x, n, d, (const int*)m.perm, m.xs, m.norm);
    return launch_status(who);
}

int rbf_fit(const float* x, int n, int d, const int* labels, int K, double gamma, double C, double tol, int max_iter, double* dual_coef,
            double* rho, int* info, hipStream_t s) {
    const long long P = (long long)K * (K - 1) / 2;
    RbfModel m;
    const size_t gram_b = rbf_up((size_t)n * n * 8), pairs_b = rbf_up((size_t)P * 8);
    int rc = rbf_group_rows("rbf_svm_fit", x, n, d, labels, K, gram_b + pairs_b, m, s);
    char* big = nullptr;                                      // the state of the pairs over RBF_LDS_ROWS rows
    std::vector<int2> pairs;
    std::vector<long long> scratch_at;
    hipError_t e = hipSuccess;
    if (rc == HSEFR_OK) {
        double* gram = (double*)m.free_bytes;
        int2* d_pairs = (int2*)(m.free_bytes + gram_b);
        rc = svm_rbf_kernel_matrix(m.xs, n, m.norm, m.xs, n, m.norm, d, gamma, gram, n, 1, "rbf_svm_fit (Gram matrix)", s);
        // the pairs by size, the largest first (a counting sort: equal sizes stay in libsvm's order)
        const std::vector<int>& st = m.h_start;
        std::vector<long long> at(n + 2, 0);
        for (int i = 0; i < K; ++i)
            for (int j = i + 1; j < K; ++j) ++at[n - (st[i + 1] - st[i] + st[j + 1] - st[j]) + 1];
        for (int v = 0; v <= n; ++v) at[v + 1] += at[v];
        pairs.resize((size_t)P);
        for (int i = 0; i < K; ++i)
            for (int j = i + 1; j < K; ++j) pairs[(size_t)at[n - (st[i + 1] - st[i] + st[j + 1] - st[j])]++] = make_int2(i, j);
        long long n_group = 0, scratch = 0;
        for (long long p = 0; p < P; ++p) {
            const int rows = st[pairs[p].x + 1] - st[pairs[p].x] + st[pairs[p].y + 1] - st[pairs[p].y];
            if (rows <= RBF_WAVE_ROWS) break;
            ++n_group;
            if (rows > RBF_LDS_ROWS) { scratch_at.push_back(scratch); scratch += 2ll * rows; }
        }
        const size_t at_b = rbf_up(scratch_at.size() * 8);
        if (rc == HSEFR_OK && !scratch_at.empty() && (hipMallocAsync((void**)&big, at_b + (size_t)scratch * 8, s) != hipSuccess || !big)) {
            (void)hipGetLastError();
            big = nullptr;
            set_error("rbf_svm_fit: no stream-ordered workspace (%zu bytes) for the %zu pairs of more than %d rows", at_b + (size_t)scratch * 8,
                      scratch_at.size(), RBF_LDS_ROWS);
            rc = HSEFR_ERR_NOMEM;
        }
        if (rc == HSEFR_OK) {
            e = hipMemcpyAsync(d_pairs, pairs.data(), (size_t)P * 8, hipMemcpyHostToDevice, s);
            if (e == hipSuccess && big) e = hipMemcpyAsync(big, scratch_at.data(), scratch_at.size() * 8, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = hipMemsetAsync(info, 0, 3 * sizeof(int), s);
        }
        if (rc == HSEFR_OK && e == hipSuccess) {
            RbfFit a{gram, n, K, m.start, m.perm, d_pairs, 0, n_group, (const long long*)big, big ? (double*)(big + at_b) : nullptr,
                     C, tol, max_iter, dual_coef, rho, info};
            if (n_group) HSEFR_LAUNCH((rbf_smo_kernel<256, RBF_LDS_ROWS, 1>), dim3((unsigned)n_group), dim3(256), 0, s, a);
            a.first = n_group; a.count = P - n_group;
            if (a.count)
                HSEFR_LAUNCH((rbf_smo_kernel<64, RBF_WAVE_ROWS, RBF_WAVE_PAIRS>), dim3((unsigned)((a.count + RBF_WAVE_PAIRS - 1) / RBF_WAVE_PAIRS)),
                             dim3(64), 0, s, a);
            HSEFR_LAUNCH(rbf_info_kernel, dim3(1), dim3(1), 0, s, info);
            rc = launch_status("rbf_svm_fit (pair solvers)");
        }
        if (e == hipSuccess) e = hipStreamSynchronize(s);     // the pair list leaves the host's memory only now
        if (rc == HSEFR_OK && e != hipSuccess) {
            set_error("rbf_svm_fit: the pair list or the solvers failed: %s", hipGetErrorString(e));
            rc = HSEFR_ERR_HIP;
        }
    }
    if (big) (void)hipFreeAsync(big, s);
    if (m.ws) (void)hipFreeAsync(m.ws, s);
    return rc;
}

// decisions (out) or labels (pred, votes) of the probes, a tile of at most RBF_TILE_Q at a time
int rbf_apply(const char* who, const float* q, int nq, const float* x, int n, int d, const int* labels, int K, double gamma,
              const double* dual_coef, const double* rho, double* out, int* pred, int* votes, hipStream_t s) {
    const long long P = (long long)K * (K - 1) / 2;
    const int ldq = nq < RBF_TILE_Q ? (nq + 63) / 64 * 64 : RBF_TILE_Q;
    std::vector<int2> tasks;
    for (int i = 0; i + 1 < K; ++i)
        for (int j = i + 1; j < K; j += RBF_OPPONENTS) tasks.push_back(make_int2(i, j));
    const size_t dcs_b = rbf_up((size_t)(K - 1) * n * 8), kqt_b = rbf_up((size_t)n * ldq * 8), qn_b = rbf_up((size_t)nq * 8),
                 votes_b = rbf_up((size_t)K * ldq * 4), tasks_b = rbf_up(tasks.size() * 8);
    RbfModel m;
    int rc = rbf_group_rows(who, x, n, d, labels, K, dcs_b + kqt_b + qn_b + votes_b + tasks_b, m, s);
    if (rc == HSEFR_OK) {
        double* dcs = (double*)m.free_bytes;
        double* kqt = (double*)(m.free_bytes + dcs_b);
        double* qn = (double*)(m.free_bytes + dcs_b + kqt_b);
        int* votes_t = (int*)(m.free_bytes + dcs_b + kqt_b + qn_b);
        int2* d_tasks = (int2*)(m.free_bytes + dcs_b + kqt_b + qn_b + votes_b);
        hipError_t e = hipMemcpyAsync(d_tasks, tasks.data(), tasks.size() * 8, hipMemcpyHostToDevice, s);
        const long long coefs = (long long)(K - 1) * n;
        HSEFR_LAUNCH(rbf_group_coef_kernel, dim3((unsigned)((coefs + 255) / 256)), dim3(256), 0, s, dual_coef, K - 1, n, (const int*)m.perm, dcs);
        HSEFR_LAUNCH(rbf_rows_kernel, dim3(nq), dim3(64), 0, s, q, nq, d, (const int*)nullptr, (float*)nullptr, qn);
        rc = launch_status(who);
        for (int q0 = 0; q0 < nq && rc == HSEFR_OK && e == hipSuccess; q0 += ldq) {
            const int count = nq - q0 < ldq ? nq - q0 : ldq;
            rc = svm_rbf_kernel_matrix(m.xs, n, m.norm, q + (long long)q0 * d, count, qn + q0, d, gamma, kqt, ldq, 0, who, s);
            if (rc != HSEFR_OK) break;
            if (pred) e = hipMemsetAsync(votes_t, 0, (size_t)K * ldq * 4, s);
            if (e != hipSuccess) break;
            const RbfVote a{kqt, dcs, rho, m.start, d_tasks, n, K, ldq, count, q0, P, pred ? votes_t : nullptr, out};
            HSEFR_LAUNCH(rbf_vote_kernel, dim3((unsigned)tasks.size(), (count + 63) / 64), dim3(64), 0, s, a);
            if (pred) HSEFR_LAUNCH(rbf_label_kernel, dim3((count + 63) / 64), dim3(64), 0, s, (const int*)votes_t, K, ldq, count, q0, pred, votes);
            rc = launch_status(who);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(s);     // the task list leaves the host's memory only now
        if (rc == HSEFR_OK && e != hipSuccess) {
            set_error("%s: a copy, a clear or a kernel failed: %s", who, hipGetErrorString(e));
            rc = HSEFR_ERR_HIP;
        }
    }
    if (m.ws) (void)hipFreeAsync(m.ws, s);
    return rc;
}

int rbf_check_model(const char* who, const void* q, int nq, const void* x, int n, int d, const void* labels, int K, double gamma,
                    const void* dual_coef, const void* rho) {
    HSEFR_REQUIRE(q && x && labels && dual_coef && rho, HSEFR_ERR_INVALID, "%s: null pointer (q %p, x %p, labels %p, dual_coef %p, rho %p)", who, q,
                  x, labels, dual_coef, rho);
    HSEFR_REQUIRE(nq >= 1 && n >= 2 && d >= 1 && K >= 2, HSEFR_ERR_INVALID, "%s: nq=%d n=%d d=%d n_classes=%d, at least 1, 2, 1 and 2 are needed",
                  who, nq, n, d, K);
    HSEFR_REQUIRE(nq <= (1 << 20) && n <= RBF_MAX_N && d <= RBF_MAX_D && K <= RBF_MAX_CLASSES && K <= n, HSEFR_ERR_INVALID,
                  "%s: nq=%d n=%d d=%d n_classes=%d over the limits nq <= %d, n <= %d, d <= %d, n_classes <= min(n, %d)", who, nq, n, d, K, 1 << 20,
                  RBF_MAX_N, RBF_MAX_D, RBF_MAX_CLASSES);
    HSEFR_REQUIRE(gamma > 0.0 && gamma <= DBL_MAX, HSEFR_ERR_INVALID, "%s: gamma=%g must be positive and finite", who, gamma);
    return HSEFR_OK;
}

}  // namespace
}  // namespace hsefr

using namespace hsefr;

#pragma GCC visibility push(default)   // the library is built with -fvisibility=hidden
extern "C" {

int hsefr_rbf_svm_gamma_scale(const float* x, int n, int d, int d_used, double* gamma, hsefr_stream_t stream) {
    HSEFR_REQUIRE(x && gamma, HSEFR_ERR_INVALID, "rbf_svm_gamma_scale: null pointer (x %p, gamma %p)", (const void*)x, (const void*)gamma);
    HSEFR_REQUIRE(n >= 1 && d >= 1 && d_used >= 1 && d_used <= d, HSEFR_ERR_INVALID,
                  "rbf_svm_gamma_scale: n=%d d=%d d_used=%d, at least 1 each and d_used <= d are needed", n, d, d_used);
    HSEFR_REQUIRE(n <= (1 << 20) && d <= RBF_MAX_D, HSEFR_ERR_INVALID, "rbf_svm_gamma_scale: n=%d d=%d over the limits n <= %d, d <= %d", n, d,
                  1 << 20, RBF_MAX_D);
    hipStream_t s = (hipStream_t)stream;
    double* ws = nullptr;
    if (hipMallocAsync((void**)&ws, 257 * sizeof(double), s) != hipSuccess || !ws) {
        (void)hipGetLastError();
        set_error("rbf_svm_gamma_scale: no stream-ordered workspace (%zu bytes)", 257 * sizeof(double));
        return HSEFR_ERR_NOMEM;
    }
    const double total = (double)n * (double)d_used;
    HSEFR_LAUNCH(rbf_moment_kernel, dim3(256), dim3(256), 0, s, x, n, d, d_used, (const double*)nullptr, ws);
    HSEFR_LAUNCH(rbf_moment_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, total, d_used, 0, ws + 256);
    HSEFR_LAUNCH(rbf_moment_kernel, dim3(256), dim3(256), 0, s, x, n, d, d_used, (const double*)(ws + 256), ws);
    HSEFR_LAUNCH(rbf_moment_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, total, d_used, 1, gamma);
    const int rc = launch_status("rbf_svm_gamma_scale");
    (void)hipFreeAsync(ws, s);
    return rc;
}

int hsefr_rbf_svm_fit(const float* x, int n, int d, const int* labels, int n_classes, double gamma, double C, double tol, int max_iter,
                      double* dual_coef, double* rho, int* info, hsefr_stream_t stream) {
    HSEFR_REQUIRE(x && labels && dual_coef && rho && info, HSEFR_ERR_INVALID,
                  "rbf_svm_fit: null pointer (x %p, labels %p, dual_coef %p, rho %p, info %p)", (const void*)x, (const void*)labels,
                  (const void*)dual_coef, (const void*)rho, (const void*)info);
    HSEFR_REQUIRE(n >= 2 && d >= 1 && n_classes >= 2, HSEFR_ERR_INVALID, "rbf_svm_fit: n=%d d=%d n_classes=%d, at least 2, 1 and 2 are needed", n, d,
                  n_classes);
    HSEFR_REQUIRE(n <= RBF_MAX_N && d <= RBF_MAX_D && n_classes <= RBF_MAX_CLASSES && n_classes <= n, HSEFR_ERR_INVALID,
                  "rbf_svm_fit: n=%d d=%d n_classes=%d over the limits n <= %d, d <= %d, n_classes <= min(n, %d)", n, d, n_classes, RBF_MAX_N,
                  RBF_MAX_D, RBF_MAX_CLASSES);
    HSEFR_REQUIRE(gamma > 0.0 && gamma <= DBL_MAX, HSEFR_ERR_INVALID, "rbf_svm_fit: gamma=%g must be positive and finite", gamma);
    HSEFR_REQUIRE(C > 0.0 && C <= DBL_MAX, HSEFR_ERR_INVALID, "rbf_svm_fit: C=%g must be positive and finite", C);
    HSEFR_REQUIRE(tol > 0.0 && tol <= DBL_MAX, HSEFR_ERR_INVALID, "rbf_svm_fit: tol=%g must be positive and finite", tol);
    HSEFR_REQUIRE(max_iter >= 1, HSEFR_ERR_INVALID, "rbf_svm_fit: max_iter=%d must be at least 1", max_iter);
    return rbf_fit(x, n, d, labels, n_classes, gamma, C, tol, max_iter, dual_coef, rho, info, (hipStream_t)stream);
}

int hsefr_rbf_svm_decision(const float* q, int nq, const float* x, int n, int d, const int* labels, int n_classes, double gamma,
                           const double* dual_coef, const double* rho, double* out, hsefr_stream_t stream) {
    const int rc = rbf_check_model("rbf_svm_decision", q, nq, x, n, d, labels, n_classes, gamma, dual_coef, rho);
    if (rc != HSEFR_OK) return rc;
    HSEFR_REQUIRE(out, HSEFR_ERR_INVALID, "rbf_svm_decision: null pointer (out %p)", (const void*)out);
    const long long P = (long long)n_classes * (n_classes - 1) / 2;
    HSEFR_REQUIRE(nq * P <= RBF_MAX_DECISIONS, HSEFR_ERR_INVALID,
                  "rbf_svm_decision: nq=%d probes x %lld pairs over the limit of %lld decision values (hsefr_rbf_svm_predict labels the probes "
                  "without them)", nq, P, RBF_MAX_DECISIONS);
    return rbf_apply("rbf_svm_decision", q, nq, x, n, d, labels, n_classes, gamma, dual_coef, rho, out, nullptr, nullptr, (hipStream_t)stream);
}

int hsefr_rbf_svm_predict(const float* q, int nq, const float* x, int n, int d, const int* labels, int n_classes, double gamma,
                          const double* dual_coef, const double* rho, int* pred, int* votes, hsefr_stream_t stream) {
    const int rc = rbf_check_model("rbf_svm_predict", q, nq, x, n, d, labels, n_classes, gamma, dual_coef, rho);
    if (rc != HSEFR_OK) return rc;
    HSEFR_REQUIRE(pred, HSEFR_ERR_INVALID, "rbf_svm_predict: null pointer (pred %p)", (const void*)pred);
    return rbf_apply("rbf_svm_predict", q, nq, x, n, d, labels, n_classes, gamma, dual_coef, rho, nullptr, pred, votes, (hipStream_t)stream);
}

}  // extern "C"
#pragma GCC visibility pop
