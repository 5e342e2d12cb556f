// sklearn.svm.LinearSVC() (facerec_test.py:269-288 'linear svm' / 'linear svm+PCA', :429) on the device, at the objective's optimum:
// hsefr_linear_svm_fit / hsefr_linear_svm_decision / hsefr_linear_svm_predict.
//
// One-vs-rest, L2 penalty, squared hinge, the bias regularised like any weight (liblinear): for class k, with x~ = (x, 1) and
// y_ik = +1 where label_i == k, else -1,
//     f_k(w~) = 1/2 |w~|^2 + C sum_i max(0, 1 - y_ik <w~, x~_i>)^2 ,
// 1-strongly convex, so |w~ - w~*| <= |grad f_k(w~)|.  All classes of a block are solved at once by a truncated Newton method in fp64.
// The vectors are stored as ROWS (W [B, d+1]) and everything per sample is class-major ([B, n]), so every product is
// out[i][j] = sum_k A(i,k) B(j,k) over strided operands -- ONE MFMA tile kernel (v_mfma_f64_16x16x4_f64), its epilogue chosen at run time:
//     S = W X~^T, R = (1 - y S > 0) ? y - S : 0        margin epilogue (f_k = 1/2 |w~|^2 + C |R_k|^2)
//     G = W - 2C R X~                                   add + alpha * acc
//     Hp = P + 2C ((R != 0) o (P X~^T)) X~              masked store, then add + alpha * acc
//     Q = D X~^T                                        plain store: f_k(w~ + t d) for every trial step t from (S, Q), no product per trial
// and one workgroup-per-class kernel does every reduction and update between the products (CG with per-class scalars, the Armijo
// search, the convergence test).  A class is converged when |grad f_k| <= tol |grad f_k(0)|; it is frozen from then on, and a tile whose
// 32 classes are all frozen (or have finished their CG) is not computed.  Every sum has a fixed shape (no floating-point atomics), the
// start is W = 0: two runs give equal bits.  The host reads 32 bytes per Newton iteration: the classes still open, and how the last
// CG went, from which it sets the number of CG steps it enqueues for the next one.
#include "common.h"
#include "svm_gemm.h"

#include <float.h>
#include <math.h>

namespace hsefr {
namespace {

typedef double svm_f64x4 __attribute__((ext_vector_type(4)));

// element (row r, summation index k) of an operand = p[r * sr + k * sk], fp64 or (f32) fp32; rows >= rows and k >= K read as zero
struct SvmOperand {
    const void* p;
    long long sr, sk;
    int rows, f32;
};
enum { SVM_EP_STORE = 0, SVM_EP_MARGIN = 1, SVM_EP_MASKED = 2, SVM_EP_AXPY = 3, SVM_EP_BIAS = 4, SVM_EP_RBF = 5 };
// out [M, ncols] with row stride ldo.  MARGIN: out = S, out2 = R, the class of row i is cls0 + i, labels [ncols].  MASKED: mask [M, ncols]
// (ldo).  AXPY: out = add + alpha * acc, add [M, ncols] (ldo).  BIAS: out = acc + bias[j].  RBF (csrc/rbf_svm.hip, through
// svm_rbf_kernel_matrix): out = exp(-alpha max(0, aux2[i] + aux[j] - 2 acc)), the squared norms of the rows of A and B; with cls0 != 0
// (libsvm's training matrix) every value is rounded to fp32 and the diagonal i == j is exactly 1.
struct SvmEpilogue {
    double* out;
    double* out2;
    long long ldo;
    int mode, ncols, cls0;
    double alpha;
    const double* aux;       // mask / add / bias
    const int* labels;
    const int* live;         // per row of the result (a class), or null: a tile without a live row is skipped
    const double* aux2;      // RBF: the squared norm of each row of A
};

constexpr int SVM_TM = 32, SVM_TN = 64, SVM_TK = 16;

__device__ __forceinline__ double svm_op_load(const SvmOperand& o, int r, int k, int K) {
    if (r >= o.rows || k >= K) return 0.0;
    const long long at = (long long)r * o.sr + (long long)k * o.sk;
    return o.f32 ? (double)((const float*)o.p)[at] : ((const double*)o.p)[at];
}
// a [R rows][SVM_TK] tile, R * 16 / 256 elements per thread, the fastest thread index along the operand's unit stride
template <int R>
__device__ __forceinline__ void svm_tile_load(const SvmOperand& o, int r0, int k0, int K, int tid, double (&v)[R / 16]) {
#pragma unroll
    for (int e = 0; e < R / 16; ++e) {
        const int idx = tid + 256 * e;
        const int r = o.sk == 1 ? idx / SVM_TK : idx % R, k = o.sk == 1 ? idx % SVM_TK : idx / R;
        v[e] = svm_op_load(o, r0 + r, k0 + k, K);
    }
}
template <int R>
__device__ __forceinline__ void svm_tile_store(const SvmOperand& o, double (*s)[R + 1], int tid, const double (&v)[R / 16]) {
#pragma unroll
    for (int e = 0; e < R / 16; ++e) {
        const int idx = tid + 256 * e;
        const int r = o.sk == 1 ? idx / SVM_TK : idx % R, k = o.sk == 1 ? idx % SVM_TK : idx / R;
        s[k][r] = v[e];
    }
}

// 256 threads = 4 waves, a 32 x 64 output tile: wave w owns rows 16 (w & 1) .. and columns 32 (w >> 1) .. (two 16 x 16 MFMA tiles).
// Lane l supplies A[row l & 15][k = l >> 4] and B[k = l >> 4][column l & 15]; result register g of lane l is row (l >> 4) + 4 g,
// column l & 15 (the f64 map).
__global__ __launch_bounds__(256) void svm_gemm_kernel(SvmOperand A, SvmOperand B, int M, int K, SvmEpilogue ep) {
    __shared__ double As[SVM_TK][SVM_TM + 1];
    __shared__ double Bs[SVM_TK][SVM_TN + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * SVM_TM, n0 = blockIdx.y * SVM_TN;
    if (ep.live) {                                            // the same answer in every thread: all leave together
        int any = 0;
        for (int i = m0; i < m0 + SVM_TM && i < M; ++i) any |= ep.live[i];
        if (!any) return;
    }
    const int wm = (wave & 1) * 16, wn = (wave >> 1) * 32;
    const int r = lane & 15, q = lane >> 4;
    svm_f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
    double va[SVM_TM / 16], vb[SVM_TN / 16];
    svm_tile_load<SVM_TM>(A, m0, 0, K, tid, va);
    svm_tile_load<SVM_TN>(B, n0, 0, K, tid, vb);
    for (int k0 = 0; k0 < K; k0 += SVM_TK) {
        __syncthreads();                                      // the previous tile has been read
        svm_tile_store<SVM_TM>(A, As, tid, va);
        svm_tile_store<SVM_TN>(B, Bs, tid, vb);
        __syncthreads();
        if (k0 + SVM_TK < K) {                                // the next tile travels while this one is multiplied
            svm_tile_load<SVM_TM>(A, m0, k0 + SVM_TK, K, tid, va);
            svm_tile_load<SVM_TN>(B, n0, k0 + SVM_TK, K, tid, vb);
        }
#pragma unroll
        for (int kk = 0; kk < SVM_TK; kk += 4) {
            const double a = As[kk + q][wm + r];
            const double b0 = Bs[kk + q][wn + r], b1 = Bs[kk + q][wn + 16 + r];
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b1, acc1, 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const svm_f64x4 acc = t ? acc1 : acc0;
        const int j = n0 + wn + 16 * t + r;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int i = m0 + wm + q + 4 * g;
            if (i >= M || j >= ep.ncols) continue;
            const long long at = (long long)i * ep.ldo + j;
            double v = acc[g];
            if (ep.mode == SVM_EP_MARGIN) {
                const double y = ep.labels[j] == ep.cls0 + i ? 1.0 : -1.0;
                ep.out2[at] = 1.0 - y * v > 0.0 ? y - v : 0.0;
            } else if (ep.mode == SVM_EP_MASKED) {
                v = ep.aux[at] != 0.0 ? v : 0.0;
            } else if (ep.mode == SVM_EP_AXPY) {
                v = ep.aux[at] + ep.alpha * v;
            } else if (ep.mode == SVM_EP_BIAS) {
                v += ep.aux[j];
            } else if (ep.mode == SVM_EP_RBF) {
                const double d2 = ep.aux2[i] + ep.aux[j] - 2.0 * v;
                v = exp(-ep.alpha * (d2 > 0.0 ? d2 : 0.0));
                if (ep.cls0) v = i == j ? 1.0 : (double)(float)v;
            }
            ep.out[at] = v;
        }
    }
}

enum { SVM_FLAG_OPEN = 0, SVM_FLAG_TRUNCATED = 1, SVM_FLAG_STEPS = 2, SVM_FLAG_MOVED = 3, SVM_FLAG_BAD_LABEL = 4, SVM_FLAGS = 8 };

// X~ [n, d + 1] fp64 = (x, 1); a label code outside 0 .. n_classes - 1 raises the flag (every writer stores the same 1)
__global__ __launch_bounds__(256) void svm_prep_kernel(const float* __restrict__ x, int n, int d, const int* __restrict__ labels,
                                                       int n_classes, double* __restrict__ xt, int* flags) {
    const long long count = (long long)n * (d + 1), i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int row = (int)(i / (d + 1)), c = (int)(i % (d + 1));
    xt[i] = c < d ? (double)x[(long long)row * d + c] : 1.0;
    if (c == d && (labels[row] < 0 || labels[row] >= n_classes)) flags[SVM_FLAG_BAD_LABEL] = 1;
}

// the sum (or maximum) over a 256-thread workgroup, in every thread, in a fixed order
__device__ double svm_block_reduce(double v, int is_max, double* part /* [4], shared */) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double u = __shfl_xor(v, o);
        v = is_max ? fmax(v, u) : v + u;
    }
    __syncthreads();                                          // the previous call's values have been read
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return is_max ? fmax(fmax(part[0], part[1]), fmax(part[2], part[3])) : (part[0] + part[1]) + (part[2] + part[3]);
}

enum { SVM_ROW_INIT = 0, SVM_ROW_CG = 1, SVM_ROW_SEARCH = 2, SVM_ROW_SUMMARY = 3, SVM_ROW_FINISH = 4 };
struct SvmRows {
    int phase, B, n, d1, cls0, first;
    double C, tol;
    double *W, *G, *D, *Rc, *P, *HP;        // [B, d1]
    const double *S, *Q;                    // [B, n]
    const int* labels;
    double *g0sq, *rs, *cgtol2;             // [B]
    int *open, *live, *steps, *truncated, *used, *moved;      // [B]
    int* flags;
    double* coef;                           // FINISH: rows row0 .. of coef [K', d1 - 1] and intercept [K']
    double* intercept;
    int row0;
    int* info;                              // FINISH of the last block: iterations, converged, Hessian-vector products
    int iterations, converged, products;
};

// Everything between the products, one workgroup per class k (SUMMARY: one workgroup in all).
//   INIT     |G_k|^2 against tol^2 |G_k(0)|^2; an open class starts its CG: D = 0, Rc = P = -G, forcing term min(0.1, sqrt(|g| / |g0|))
//   CG       one step from Hp: alpha = rs / <P, Hp>, D += alpha P, Rc -= alpha Hp; done at |Rc| <= forcing * |g|, else P = Rc + beta P
//   SEARCH   the largest t = 2^-m with f(W + t D) - f(W) <= 1e-4 t <G, D>, the difference summed term by term (never as two objectives:
//            near the optimum it is far below their rounding); W += t D
//   SUMMARY  the flags the host reads
//   FINISH   coef / intercept rows (and info)
__global__ __launch_bounds__(256) void svm_rows_kernel(SvmRows a) {
    __shared__ double part[4];
    const int k = blockIdx.x, tid = threadIdx.x;
    const long long w0 = (long long)k * a.d1;
    if (a.phase == SVM_ROW_INIT) {
        if (!a.first && !a.open[k]) return;
        double gs = 0.0;
        for (int c = tid; c < a.d1; c += 256) gs += a.G[w0 + c] * a.G[w0 + c];
        gs = svm_block_reduce(gs, 0, part);
        const double g0 = a.first ? gs : a.g0sq[k];
        const int open = gs <= a.tol * a.tol * g0 ? 0 : 1;     // a NaN stays open
        if (tid == 0) {
            if (a.first) a.g0sq[k] = gs;
            a.open[k] = open;
            a.live[k] = open;
            a.steps[k] = 0;
            a.rs[k] = gs;
            const double ratio = sqrt(gs / g0);
            a.cgtol2[k] = (ratio < 0.01 ? ratio : 0.01) * gs;  // (min(0.1, sqrt(|g| / |g0|)) |g|)^2
        }
        if (open)
            for (int c = tid; c < a.d1; c += 256) {
                const double g = a.G[w0 + c];
                a.D[w0 + c] = 0.0;
                a.Rc[w0 + c] = -g;
                a.P[w0 + c] = -g;
            }
    } else if (a.phase == SVM_ROW_CG) {
        if (!a.live[k]) return;
        const double rs = a.rs[k];
        double php = 0.0;
        for (int c = tid; c < a.d1; c += 256) php += a.P[w0 + c] * a.HP[w0 + c];
        php = svm_block_reduce(php, 0, part);
        if (!(php > 0.0)) {                                    // H is positive definite: only values that are not finite come here
            if (tid == 0) a.live[k] = 0;
            return;
        }
        const double alpha = rs / php;
        double rsn = 0.0;
        for (int c = tid; c < a.d1; c += 256) {
            a.D[w0 + c] += alpha * a.P[w0 + c];
            const double r = a.Rc[w0 + c] - alpha * a.HP[w0 + c];
            a.Rc[w0 + c] = r;
            rsn += r * r;
        }
        rsn = svm_block_reduce(rsn, 0, part);
        const int done = rsn <= a.cgtol2[k] ? 1 : 0;
        if (!done) {
            const double beta = rsn / rs;
            for (int c = tid; c < a.d1; c += 256) a.P[w0 + c] = a.Rc[w0 + c] + beta * a.P[w0 + c];
        }
        if (tid == 0) {
            a.rs[k] = rsn;
            a.steps[k] += 1;
            if (done) a.live[k] = 0;
        }
    } else if (a.phase == SVM_ROW_SEARCH) {
        if (!a.open[k]) {
            if (tid == 0) { a.truncated[k] = 0; a.used[k] = 0; a.moved[k] = 0; }
            return;
        }
        double wd = 0.0, dd = 0.0, gd = 0.0;
        for (int c = tid; c < a.d1; c += 256) {
            const double d = a.D[w0 + c];
            wd += a.W[w0 + c] * d;
            dd += d * d;
            gd += a.G[w0 + c] * d;
        }
        wd = svm_block_reduce(wd, 0, part);
        dd = svm_block_reduce(dd, 0, part);
        gd = svm_block_reduce(gd, 0, part);
        double t = 1.0;
        int accepted = 0;
        if (gd < 0.0) {
            const int cls = a.cls0 + k;
            const double* s = a.S + (long long)k * a.n;
            const double* q = a.Q + (long long)k * a.n;
            for (int trial = 0; trial < 60 && !accepted; ++trial) {
                double sum = 0.0;
                for (int i = tid; i < a.n; i += 256) {
                    const double y = a.labels[i] == cls ? 1.0 : -1.0;
                    const double m = 1.0 - y * s[i], b = t * y * q[i], m2 = m - b;       // the margin's slack before and after
                    if (m > 0.0 && m2 > 0.0) sum += b * (b - 2.0 * m);
                    else sum += (m2 > 0.0 ? m2 * m2 : 0.0) - (m > 0.0 ? m * m : 0.0);
                }
                sum = svm_block_reduce(sum, 0, part);
                const double delta = t * wd + 0.5 * t * t * dd + a.C * sum;
                if (delta <= 1e-4 * t * gd) accepted = 1;
                else t *= 0.5;
            }
        }
        if (accepted)
            for (int c = tid; c < a.d1; c += 256) a.W[w0 + c] += t * a.D[w0 + c];
        if (tid == 0) {
            a.truncated[k] = a.live[k];
            a.used[k] = a.steps[k];
            a.moved[k] = accepted;
        }
    } else if (a.phase == SVM_ROW_SUMMARY) {
        double open = 0.0, trunc = 0.0, used = 0.0, moved = 0.0;
        for (int c = tid; c < a.B; c += 256) {
            open += (double)a.open[c];
            trunc += (double)a.truncated[c];
            used = fmax(used, (double)a.used[c]);
            moved += (double)a.moved[c];
        }
        open = svm_block_reduce(open, 0, part);
        trunc = svm_block_reduce(trunc, 0, part);
        used = svm_block_reduce(used, 1, part);
        moved = svm_block_reduce(moved, 0, part);
        if (tid == 0) {
            a.flags[SVM_FLAG_OPEN] = (int)open;
            a.flags[SVM_FLAG_TRUNCATED] = (int)trunc;
            a.flags[SVM_FLAG_STEPS] = (int)used;
            a.flags[SVM_FLAG_MOVED] = (int)moved;
        }
    } else {
        const int d = a.d1 - 1;
        for (int c = tid; c < d; c += 256) a.coef[(long long)(a.row0 + k) * d + c] = a.W[w0 + c];
        if (tid == 0) {
            a.intercept[a.row0 + k] = a.W[w0 + d];
            if (k == 0 && a.info) { a.info[0] = a.iterations; a.info[1] = a.converged; a.info[2] = a.products; }
        }
    }
}

// arg-max of each row of decision [n, K], exact ties to the lowest index (np.argmax); K == 1: decision > 0.  A wave per row.
__global__ __launch_bounds__(256) void svm_predict_kernel(const double* __restrict__ dec, int n, int K, int* __restrict__ pred) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    const double* v = dec + (long long)row * K;
    if (K == 1) {
        if (lane == 0) pred[row] = v[0] > 0.0 ? 1 : 0;
        return;
    }
    double best = v[0];                                       // index 0 unless a later value is greater
    int at = 0;
    for (int c = lane; c < K; c += 64)
        if (v[c] > best) { best = v[c]; at = c; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const int oa = __shfl_xor(at, o);
        if (ob > best || (ob == best && oa < at)) { best = ob; at = oa; }
    }
    if (lane == 0) pred[row] = at;
}

size_t svm_up16(size_t b) { return (b + 15) & ~(size_t)15; }

int svm_gemm(const SvmOperand& A, const SvmOperand& B, int M, int N, int K, const SvmEpilogue& ep, const char* what, hipStream_t s) {
    const dim3 grid((M + SVM_TM - 1) / SVM_TM, (N + SVM_TN - 1) / SVM_TN);
    HSEFR_LAUNCH(svm_gemm_kernel, grid, dim3(256), 0, s, A, B, M, K, ep);
    return launch_status(what);
}

SvmOperand svm_rows_of(const double* p, int rows, long long ld) { return SvmOperand{p, ld, 1, rows, 0}; }        // (r, k) = p[r][k]
SvmOperand svm_cols_of(const double* p, int cols, long long ld) { return SvmOperand{p, 1, ld, cols, 0}; }        // (r, k) = p[k][r]

// the limits of the three entry points: the LFW half split (4582 x 1024, 1680 classes) is far inside
constexpr int SVM_MAX_N = 1 << 20, SVM_MAX_D = 1 << 14, SVM_MAX_CLASSES = 1 << 16;
constexpr long long SVM_MAX_ELEMS = 1ll << 30;                // n (d + 1) and n K': 8 GiB of fp64
constexpr int SVM_BLOCK = 512;                                // classes solved at once
constexpr int SVM_CG_FIRST = 16, SVM_CG_CAP = 1024;

int svm_fit(const float* x, int n, int d, const int* labels, int n_classes, double C, double tol, int max_iter, double* coef,
            double* intercept, int* info, hipStream_t s) {
    const int d1 = d + 1, rows = n_classes == 2 ? 1 : n_classes;
    const int nblocks = (rows + SVM_BLOCK - 1) / SVM_BLOCK, B = (rows + nblocks - 1) / nblocks;
    const size_t xt_bytes = svm_up16((size_t)n * d1 * 8), bn = svm_up16((size_t)B * n * 8), bd = svm_up16((size_t)B * d1 * 8);
    const size_t b8 = svm_up16((size_t)B * 8), b4 = svm_up16((size_t)B * 4);
    const size_t rest = 3 * bn + 6 * bd + 3 * b8 + 6 * b4 + SVM_FLAGS * 4;
    char* ws = nullptr;
    if (hipMallocAsync((void**)&ws, xt_bytes + rest, s) != hipSuccess || !ws) {
        (void)hipGetLastError();
        set_error("linear_svm_fit: no stream-ordered workspace (%zu bytes: the %d x %d fp64 rows and three %d x %d blocks) for n=%d d=%d "
                  "n_classes=%d", xt_bytes + rest, n, d1, B, n, n, d, n_classes);
        return HSEFR_ERR_NOMEM;
    }
    char* p = ws;
    auto take = [&p](size_t nbytes) { char* q = p; p += nbytes; return q; };
    double* Xt = (double*)take(xt_bytes);
    double* S = (double*)take(bn);
    double* R = (double*)take(bn);
    double* T = (double*)take(bn);
    SvmRows a{};
    a.B = B; a.n = n; a.d1 = d1; a.C = C; a.tol = tol; a.labels = labels;
    a.W = (double*)take(bd); a.G = (double*)take(bd); a.D = (double*)take(bd); a.Rc = (double*)take(bd); a.P = (double*)take(bd);
    a.HP = (double*)take(bd);
    a.g0sq = (double*)take(b8); a.rs = (double*)take(b8); a.cgtol2 = (double*)take(b8);
    a.open = (int*)take(b4); a.live = (int*)take(b4); a.steps = (int*)take(b4); a.truncated = (int*)take(b4); a.used = (int*)take(b4);
    a.moved = (int*)take(b4);
    a.flags = (int*)take(SVM_FLAGS * 4);
    a.S = S; a.Q = T; a.coef = coef; a.intercept = intercept;

    int rc = HSEFR_OK, host_flags[SVM_FLAGS] = {0};
    hipError_t e = hipSuccess;
    const auto read_flags = [&]() {
        e = hipMemcpyAsync(host_flags, a.flags, sizeof(host_flags), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    };
    const auto rows_phase = [&](int phase, int blocks, const char* what) {
        a.phase = phase;
        HSEFR_LAUNCH(svm_rows_kernel, dim3(blocks), dim3(256), 0, s, a);
        rc = launch_status(what);
    };
    e = hipMemsetAsync(ws + xt_bytes, 0, rest, s);
    if (e == hipSuccess) {
        const long long count = (long long)n * d1;
        HSEFR_LAUNCH(svm_prep_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, x, n, d, labels, n_classes, Xt, a.flags);
        rc = launch_status("linear_svm_fit (fp64 rows)");
        if (rc == HSEFR_OK) read_flags();
    }
    if (rc == HSEFR_OK && e == hipSuccess && host_flags[SVM_FLAG_BAD_LABEL]) {
        set_error("linear_svm_fit: a label code is outside 0..%d (n=%d d=%d)", n_classes - 1, n, d);
        rc = HSEFR_ERR_INVALID;
    }
    int iterations = 0, converged = 1, products = 0;
    for (int blk = 0; blk < nblocks && rc == HSEFR_OK && e == hipSuccess; ++blk) {
        const int row0 = blk * B, kb = rows - row0 < B ? rows - row0 : B;
        a.B = kb; a.row0 = row0; a.cls0 = rows == 1 ? 1 : row0;
        if (blk > 0) e = hipMemsetAsync(ws + xt_bytes, 0, rest, s);        // W = 0 and every per-class state
        if (e != hipSuccess) break;
        const SvmOperand X_rows = svm_rows_of(Xt, n, d1), X_cols = svm_cols_of(Xt, d1, d1);
        int it = 0, budget = SVM_CG_FIRST, done = 0;
        while (rc == HSEFR_OK) {
            SvmEpilogue ep{S, R, n, SVM_EP_MARGIN, n, a.cls0, 0.0, nullptr, labels, it ? a.open : nullptr};
            rc = svm_gemm(svm_rows_of(a.W, kb, d1), X_rows, kb, n, d1, ep, "linear_svm_fit (margins)", s);
            if (rc != HSEFR_OK) break;
            ep = SvmEpilogue{a.G, nullptr, d1, SVM_EP_AXPY, d1, 0, -2.0 * C, a.W, nullptr, it ? a.open : nullptr};
            rc = svm_gemm(svm_rows_of(R, kb, n), X_cols, kb, d1, n, ep, "linear_svm_fit (gradient)", s);
            if (rc != HSEFR_OK) break;
            a.first = it == 0;
            rows_phase(SVM_ROW_INIT, kb, "linear_svm_fit (convergence test)");
            if (rc == HSEFR_OK) rows_phase(SVM_ROW_SUMMARY, 1, "linear_svm_fit (flags)");
            if (rc != HSEFR_OK) break;
            read_flags();
            if (e != hipSuccess) break;
            if (host_flags[SVM_FLAG_OPEN] == 0) { done = 1; break; }
            if (it >= max_iter || (it > 0 && host_flags[SVM_FLAG_MOVED] == 0)) break;      // no class moved: nothing would change again
            if (it > 0) {                                       // twice what the slowest class needed, or twice the budget it did not fit in
                const int need = host_flags[SVM_FLAG_TRUNCATED] ? budget : host_flags[SVM_FLAG_STEPS];
                budget = 2 * need < SVM_CG_FIRST ? SVM_CG_FIRST : (2 * need > SVM_CG_CAP ? SVM_CG_CAP : 2 * need);
            }
            for (int step = 0; step < budget && rc == HSEFR_OK; ++step) {
                ep = SvmEpilogue{T, nullptr, n, SVM_EP_MASKED, n, 0, 0.0, R, nullptr, a.live};
                rc = svm_gemm(svm_rows_of(a.P, kb, d1), X_rows, kb, n, d1, ep, "linear_svm_fit (X p)", s);
                if (rc != HSEFR_OK) break;
                ep = SvmEpilogue{a.HP, nullptr, d1, SVM_EP_AXPY, d1, 0, 2.0 * C, a.P, nullptr, a.live};
                rc = svm_gemm(svm_rows_of(T, kb, n), X_cols, kb, d1, n, ep, "linear_svm_fit (H p)", s);
                if (rc == HSEFR_OK) rows_phase(SVM_ROW_CG, kb, "linear_svm_fit (CG step)");
                ++products;
            }
            if (rc != HSEFR_OK) break;
            ep = SvmEpilogue{T, nullptr, n, SVM_EP_STORE, n, 0, 0.0, nullptr, nullptr, a.open};
            rc = svm_gemm(svm_rows_of(a.D, kb, d1), X_rows, kb, n, d1, ep, "linear_svm_fit (X d)", s);
            if (rc == HSEFR_OK) rows_phase(SVM_ROW_SEARCH, kb, "linear_svm_fit (line search)");
            ++it;
        }
        if (rc != HSEFR_OK || e != hipSuccess) break;
        iterations = it > iterations ? it : iterations;
        converged = converged && done;
        a.info = blk == nblocks - 1 ? info : nullptr;
        a.iterations = iterations; a.converged = converged; a.products = products;
        rows_phase(SVM_ROW_FINISH, kb, "linear_svm_fit (coefficients)");
    }
    if (rc == HSEFR_OK && e != hipSuccess) {
        set_error("linear_svm_fit: clearing the workspace or reading the flags failed: %s", hipGetErrorString(e));
        rc = HSEFR_ERR_HIP;
    }
    (void)hipFreeAsync(ws, s);
    return rc;
}

}  // namespace

int svm_rbf_kernel_matrix(const float* a, int ma, const double* norm_a, const float* b, int mb, const double* norm_b, int d, double gamma,
                          double* out, long long ldo, int training, const char* what, hipStream_t s) {
    const SvmOperand ar{a, d, 1, ma, 1}, br{b, d, 1, mb, 1};
    const SvmEpilogue ep{out, nullptr, ldo, SVM_EP_RBF, mb, training, gamma, norm_b, nullptr, nullptr, norm_a};
    return svm_gemm(ar, br, ma, mb, d, ep, what, s);
}

}  // namespace hsefr

using namespace hsefr;

#pragma GCC visibility push(default)   // the library is built with -fvisibility=hidden
extern "C" {

int hsefr_linear_svm_fit(const float* x, int n, int d, const int* labels, int n_classes, double C, double tol, int max_iter, double* coef,
                         double* intercept, int* info, hsefr_stream_t stream) {
    HSEFR_REQUIRE(x && labels && coef && intercept && info, HSEFR_ERR_INVALID,
                  "linear_svm_fit: null pointer (x %p, labels %p, coef %p, intercept %p, info %p)", (const void*)x, (const void*)labels,
                  (const void*)coef, (const void*)intercept, (const void*)info);
    HSEFR_REQUIRE(n >= 1 && d >= 1 && n_classes >= 2, HSEFR_ERR_INVALID, "linear_svm_fit: n=%d d=%d n_classes=%d, at least 1, 1 and 2 are needed",
                  n, d, n_classes);
    HSEFR_REQUIRE(n <= SVM_MAX_N && d <= SVM_MAX_D && n_classes <= SVM_MAX_CLASSES && (long long)n * (d + 1) <= SVM_MAX_ELEMS,
                  HSEFR_ERR_INVALID, "linear_svm_fit: n=%d d=%d n_classes=%d over the limits n <= %d, d <= %d, n_classes <= %d, n (d + 1) <= %lld",
                  n, d, n_classes, SVM_MAX_N, SVM_MAX_D, SVM_MAX_CLASSES, SVM_MAX_ELEMS);
    HSEFR_REQUIRE(C > 0.0 && C <= DBL_MAX, HSEFR_ERR_INVALID, "linear_svm_fit: C=%g must be positive and finite", C);
    HSEFR_REQUIRE(tol > 0.0, HSEFR_ERR_INVALID, "linear_svm_fit: tol=%g must be positive", tol);
    HSEFR_REQUIRE(max_iter >= 1, HSEFR_ERR_INVALID, "linear_svm_fit: max_iter=%d must be at least 1", max_iter);
    return svm_fit(x, n, d, labels, n_classes, C, tol, max_iter, coef, intercept, info, (hipStream_t)stream);
}

int hsefr_linear_svm_decision(const float* x, int n, int d, const double* coef, const double* intercept, int k_rows, double* out,
                              hsefr_stream_t stream) {
    HSEFR_REQUIRE(x && coef && intercept && out, HSEFR_ERR_INVALID, "linear_svm_decision: null pointer (x %p, coef %p, intercept %p, out %p)",
                  (const void*)x, (const void*)coef, (const void*)intercept, (const void*)out);
    HSEFR_REQUIRE(n >= 1 && d >= 1 && k_rows >= 1, HSEFR_ERR_INVALID, "linear_svm_decision: n=%d d=%d k_rows=%d, at least 1 each is needed", n, d,
                  k_rows);
    HSEFR_REQUIRE(n <= SVM_MAX_N && d <= SVM_MAX_D && k_rows <= SVM_MAX_CLASSES && (long long)n * k_rows <= SVM_MAX_ELEMS, HSEFR_ERR_INVALID,
                  "linear_svm_decision: n=%d d=%d k_rows=%d over the limits n <= %d, d <= %d, k_rows <= %d, n k_rows <= %lld", n, d, k_rows,
                  SVM_MAX_N, SVM_MAX_D, SVM_MAX_CLASSES, SVM_MAX_ELEMS);
    const SvmOperand xr{x, d, 1, n, 1};
    const SvmEpilogue ep{out, nullptr, k_rows, SVM_EP_BIAS, k_rows, 0, 0.0, intercept, nullptr, nullptr};
    return svm_gemm(xr, svm_rows_of(coef, k_rows, d), n, k_rows, d, ep, "linear_svm_decision", (hipStream_t)stream);
}

int hsefr_linear_svm_predict(const double* decision, int n, int k_rows, int* pred, hsefr_stream_t stream) {
    HSEFR_REQUIRE(decision && pred, HSEFR_ERR_INVALID, "linear_svm_predict: null pointer (decision %p, pred %p)", (const void*)decision,
                  (const void*)pred);
    HSEFR_REQUIRE(n >= 1 && k_rows >= 1, HSEFR_ERR_INVALID, "linear_svm_predict: n=%d k_rows=%d, at least 1 each is needed", n, k_rows);
    HSEFR_REQUIRE(n <= SVM_MAX_N && k_rows <= SVM_MAX_CLASSES && (long long)n * k_rows <= SVM_MAX_ELEMS, HSEFR_ERR_INVALID,
                  "linear_svm_predict: n=%d k_rows=%d over the limits n <= %d, k_rows <= %d, n k_rows <= %lld", n, k_rows, SVM_MAX_N,
                  SVM_MAX_CLASSES, SVM_MAX_ELEMS);
    HSEFR_LAUNCH(svm_predict_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, decision, n, k_rows, pred);
    return launch_status("linear_svm_predict");
}

}  // extern "C"
#pragma GCC visibility pop
