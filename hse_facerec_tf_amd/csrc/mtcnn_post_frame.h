// The one-frame bodies of MTCNN's box logic on the device (see mtcnn_post.hip for the parity contract): the candidate lists in LDS,
// the bitonic sort, the greedy NMS and the stage bodies, each a __device__ function of ONE frame's pointers run by one workgroup of
// NT threads with sizeof(PostLds) bytes of dynamic LDS.  mtcnn_post.hip (libhsefr.so: a frame is a grid index of a same-size
// stack) and mtcnn_ragged.hip (libhsefr_ragged.so: a frame's sizes and pointers come from a table) compile this same code, so a
// frame's numbers are the same whichever entry ran it.
#pragma once
#include <hip/hip_runtime.h>

namespace hsefr {

namespace {

constexpr int CAP = 2048;          // candidates per list (per pyramid level; all levels' survivors; stage-2 / stage-3 inputs)
constexpr int NT = 1024;

struct PostLds {
    unsigned long long key[CAP];   // (0xFFFFFFFF - score bits) << 32 | (0xFFFFFFFF - index): ascending = score descending, index descending
    double x1[CAP], y1[CAP], x2[CAP], y2[CAP], area[CAP];   // in SORTED order
    unsigned char alive[CAP], kept[CAP];
    int n, nkeep;
    int keep_pos[CAP];             // sorted positions of the kept boxes, in pick order
};

__device__ __forceinline__ double dfix(double v) { return trunc(v); }
__device__ __forceinline__ double mad_sep(double a, double b, double c) { return __dadd_rn(a, __dmul_rn(b, c)); }   // a + b * c, two roundings

// bitonic sort of key[0 .. np2) ascending (np2 = power of two >= n, padded with all-ones keys)
__device__ void sort_keys(PostLds& L, int np2) {
    const int tid = threadIdx.x;
    for (int k = 2; k <= np2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < np2; i += NT) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long a = L.key[i], b = L.key[ixj];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) { L.key[i] = b; L.key[ixj] = a; }
                }
            }
            __syncthreads();
        }
}

// greedy NMS over the sorted boxes in LDS (x1..y2, area filled for positions 0 .. n-1): kept[] and keep_pos[] / nkeep
__device__ void nms_sorted(PostLds& L, int n, double thr, bool use_min) {
    const int tid = threadIdx.x;
    for (int i = tid; i < n; i += NT) { L.alive[i] = 1; L.kept[i] = 0; }
    if (tid == 0) L.nkeep = 0;
    __syncthreads();
    for (int i = 0; i < n; ++i) {
        if (!L.alive[i]) continue;                        // LDS broadcast read: uniform across the workgroup
        const double tx1 = L.x1[i], ty1 = L.y1[i], tx2 = L.x2[i], ty2 = L.y2[i], ta = L.area[i];
        for (int j = i + 1 + tid; j < n; j += NT) {
            if (!L.alive[j]) continue;
            const double iw = fmax(0.0, fmin(tx2, L.x2[j]) - fmax(tx1, L.x1[j]) + 1.0);
            const double ih = fmax(0.0, fmin(ty2, L.y2[j]) - fmax(ty1, L.y1[j]) + 1.0);
            const double inter = __dmul_rn(iw, ih);
            const double den = use_min ? fmin(ta, L.area[j]) : __dadd_rn(__dadd_rn(ta, L.area[j]), -inter);
            if (!(inter / den <= thr)) L.alive[j] = 0;
        }
        if (tid == 0) { L.kept[i] = 1; L.keep_pos[L.nkeep++] = i; }
        __syncthreads();
    }
    __syncthreads();
}

// Sort key: ascending key = descending score, and among bit-equal scores DESCENDING index -- what the reference's own
// `I = np.argsort(s)` + "pick I[-1]" does on its usual list sizes (NumPy's introsort finishes lists of <= 16 elements with a
// stable insertion sort, facial_analysis.py:398-403), made the rule for every size so the order is deterministic.
__device__ __forceinline__ unsigned long long make_key(float score, unsigned idx) {
    return ((unsigned long long)(0xFFFFFFFFu - __float_as_uint(score)) << 32) | (0xFFFFFFFFu - idx);
}
__device__ __forceinline__ unsigned key_idx(unsigned long long key) { return 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull); }
__device__ __forceinline__ int np2_of(int n) {
    int p = 2;
    while (p < n) p <<= 1;
    return p;
}

// the source window of a box clipped to the frame and where it lands in the box-sized tile (pad(), :432-466): table row
// {x1, y1, x2, y2, tx1, ty1, bw, bh} as hsefr_mtcnn_crops takes it
__device__ void crop_row(const double* b, int img_w, int img_h, int* t) {
    const int bw = (int)(b[2] - b[0] + 1.0), bh = (int)(b[3] - b[1] + 1.0);
    int x1 = (int)b[0], y1 = (int)b[1], x2 = (int)b[2], y2 = (int)b[3];
    int tx1 = 1, ty1 = 1;
    if (x2 > img_w) x2 = img_w;
    if (y2 > img_h) y2 = img_h;
    if (x1 < 1) { tx1 = 2 - x1; x1 = 1; }
    if (y1 < 1) { ty1 = 2 - y1; y1 = 1; }
    t[0] = x1; t[1] = y1; t[2] = x2; t[3] = y2; t[4] = tx1; t[5] = ty1; t[6] = bw; t[7] = bh;
}

// rerec(): square box around the centre
__device__ void square_box(double& x1, double& y1, double& x2, double& y2) {
    const double w = x2 - x1, h = y2 - y1, side = fmax(w, h);
    x1 = __dadd_rn(mad_sep(x1, w, 0.5), -__dmul_rn(side, 0.5));
    y1 = __dadd_rn(mad_sep(y1, h, 0.5), -__dmul_rn(side, 0.5));
    x2 = x1 + side;
    y2 = y1 + side;
}

// counters: [0] boxes found by stage 1 so far (all levels), [1] boxes after stage 1, [2] after stage 2, [3] after stage 3, [4] overflow
extern __shared__ unsigned char post_smem[];

// ---- stage 1, one pyramid level: threshold the face map, boxes of the firing cells, NMS 0.5, append the survivors ----------------
// (the bodies are __device__ functions of ONE frame's pointers; the __global__ entries hand a workgroup the rows of its frame)
__device__ __forceinline__ void stage1_level_frame(const float* __restrict__ prob /*[w,h,2]*/, const float* __restrict__ reg /*[w,h,4]*/, int w, int h,
                                                   double scale, float thr, double* __restrict__ found /*[CAP,9]*/, int* __restrict__ counters) {
    PostLds& L = *(PostLds*)post_smem;
    const int tid = threadIdx.x;
    if (tid == 0) L.n = 0;
    __syncthreads();
    const int cells = w * h;
    for (int i = tid; i < cells; i += NT) {
        const float s = prob[2 * i + 1];
        if (s >= thr) {
            const int pos = atomicAdd(&L.n, 1);
            if (pos < CAP) L.key[pos] = make_key(s, (unsigned)i);
        }
    }
    __syncthreads();
    const int n = L.n;
    if (n == 0) return;
    if (n > CAP) { if (tid == 0) counters[4] = 1; return; }
    const int p2 = np2_of(n);
    for (int i = n + tid; i < p2; i += NT) L.key[i] = ~0ull;
    __syncthreads();
    sort_keys(L, p2);
    for (int i = tid; i < n; i += NT) {
        const unsigned idx = key_idx(L.key[i]);
        const int xi = (int)(idx / (unsigned)h), yi = (int)(idx - (unsigned)xi * (unsigned)h);
        L.x1[i] = dfix((double)(2 * xi + 1) / scale);
        L.y1[i] = dfix((double)(2 * yi + 1) / scale);
        L.x2[i] = dfix((double)(2 * xi + 12) / scale);
        L.y2[i] = dfix((double)(2 * yi + 12) / scale);
        L.area[i] = __dmul_rn(L.x2[i] - L.x1[i] + 1.0, L.y2[i] - L.y1[i] + 1.0);
    }
    __syncthreads();
    nms_sorted(L, n, 0.5, false);
    const int base = counters[0], nk = L.nkeep;
    if (base + nk > CAP) { if (tid == 0) counters[4] = 1; return; }
    for (int k = tid; k < nk; k += NT) {
        const int i = L.keep_pos[k];
        const unsigned idx = key_idx(L.key[i]);
        const int xi = (int)(idx / (unsigned)h), yi = (int)(idx - (unsigned)xi * (unsigned)h);
        // the reference reads the regression maps flipped when exactly one cell fires (facial_analysis.py:383-387)
        const int rxi = n == 1 ? w - 1 - xi : xi;
        const float* r = reg + ((size_t)rxi * h + yi) * 4;
        double* o = found + (size_t)(base + k) * 9;
        o[0] = L.x1[i]; o[1] = L.y1[i]; o[2] = L.x2[i]; o[3] = L.y2[i];
        o[4] = (double)prob[2 * idx + 1];
        o[5] = (double)r[0]; o[6] = (double)r[1]; o[7] = (double)r[2]; o[8] = (double)r[3];
    }
    __syncthreads();
    if (tid == 0) counters[0] = base + nk;
}

// ---- stage 1, after the last level: NMS 0.7 over all survivors, regression by the P-Net offsets, square, truncate, crop windows ----
__device__ __forceinline__ void stage1_finish_frame(const double* __restrict__ found, int* __restrict__ counters, double* __restrict__ boxes /*[CAP,5]*/,
                                                    int* __restrict__ tab /*[CAP,8]*/, int img_w, int img_h) {
    PostLds& L = *(PostLds*)post_smem;
    const int tid = threadIdx.x;
    const int n = counters[0];
    if (n == 0 || counters[4]) { if (tid == 0) counters[1] = 0; return; }
    const int p2 = np2_of(n);
    for (int i = tid; i < p2; i += NT) L.key[i] = i < n ? make_key((float)found[(size_t)i * 9 + 4], (unsigned)i) : ~0ull;
    __syncthreads();
    sort_keys(L, p2);
    for (int i = tid; i < n; i += NT) {
        const double* b = found + (size_t)key_idx(L.key[i]) * 9;
        L.x1[i] = b[0]; L.y1[i] = b[1]; L.x2[i] = b[2]; L.y2[i] = b[3];
        L.area[i] = __dmul_rn(b[2] - b[0] + 1.0, b[3] - b[1] + 1.0);
    }
    __syncthreads();
    nms_sorted(L, n, 0.7, false);
    const int nk = L.nkeep;
    for (int k = tid; k < nk; k += NT) {
        const double* b = found + (size_t)key_idx(L.key[L.keep_pos[k]]) * 9;
        const double rw = b[2] - b[0], rh = b[3] - b[1];
        double x1 = mad_sep(b[0], b[5], rw), y1 = mad_sep(b[1], b[6], rh), x2 = mad_sep(b[2], b[7], rw), y2 = mad_sep(b[3], b[8], rh);
        square_box(x1, y1, x2, y2);
        double* o = boxes + (size_t)k * 5;
        o[0] = dfix(x1); o[1] = dfix(y1); o[2] = dfix(x2); o[3] = dfix(y2); o[4] = b[4];
        crop_row(o, img_w, img_h, tab + (size_t)k * 8);
    }
    if (tid == 0) counters[1] = nk;
}

// ---- stage 2 / 3 after the net: score filter, NMS 0.7, regression, (stage 2) square + truncate + crop windows, (stage 3) landmarks ----
// STAGE 2: boxes_out [m,5] = truncated square boxes (score column truncated too, as np.fix(boxes) does), tab_out rows.
// STAGE 3: regression BEFORE the NMS ('Min' overlap), boxes_out = regressed boxes + score, points_out [m,10] float32.
template <int STAGE>
__device__ __forceinline__ void stage23_finish_frame(const double* __restrict__ boxes_in /*[n,5]*/, int n, const float* __restrict__ prob /*[n,2]*/,
                                                     const float* __restrict__ reg /*[n,4]*/, const float* __restrict__ pts /*[n,10]*/, float thr,
                                                     double* __restrict__ boxes_out, int* __restrict__ tab_out, float* __restrict__ points_out,
                                                     int* __restrict__ counters, int img_w, int img_h) {
    PostLds& L = *(PostLds*)post_smem;
    const int tid = threadIdx.x;
    if (tid == 0) L.n = 0;
    __syncthreads();
    if (n > CAP) { if (tid == 0) { counters[4] = 1; counters[STAGE] = 0; } return; }
    for (int i = tid; i < n; i += NT) {
        const float s = prob[2 * i + 1];
        if (s > thr) L.key[atomicAdd(&L.n, 1)] = make_key(s, (unsigned)i);
    }
    __syncthreads();
    const int m = L.n;
    if (m == 0) { if (tid == 0) counters[STAGE] = 0; return; }
    const int p2 = np2_of(m);
    for (int i = m + tid; i < p2; i += NT) L.key[i] = ~0ull;
    __syncthreads();
    sort_keys(L, p2);
    for (int i = tid; i < m; i += NT) {
        const unsigned src = key_idx(L.key[i]);
        const double* b = boxes_in + (size_t)src * 5;
        double x1 = b[0], y1 = b[1], x2 = b[2], y2 = b[3];
        if (STAGE == 3) {      // bbreg before the NMS
            const double bw = x2 - x1 + 1.0, bh = y2 - y1 + 1.0;
            const float* r = reg + (size_t)src * 4;
            const double ox1 = x1, oy1 = y1, ox2 = x2, oy2 = y2;
            x1 = mad_sep(ox1, (double)r[0], bw); y1 = mad_sep(oy1, (double)r[1], bh);
            x2 = mad_sep(ox2, (double)r[2], bw); y2 = mad_sep(oy2, (double)r[3], bh);
        }
        L.x1[i] = x1; L.y1[i] = y1; L.x2[i] = x2; L.y2[i] = y2;
        L.area[i] = __dmul_rn(x2 - x1 + 1.0, y2 - y1 + 1.0);
    }
    __syncthreads();
    nms_sorted(L, m, 0.7, STAGE == 3);
    const int nk = L.nkeep;
    for (int k = tid; k < nk; k += NT) {
        const int i = L.keep_pos[k];
        const unsigned src = key_idx(L.key[i]);
        const float score = prob[2 * src + 1];
        double* o = boxes_out + (size_t)k * 5;
        if (STAGE == 2) {
            const double* b = boxes_in + (size_t)src * 5;
            const double bw = b[2] - b[0] + 1.0, bh = b[3] - b[1] + 1.0;
            const float* r = reg + (size_t)src * 4;
            double x1 = mad_sep(b[0], (double)r[0], bw), y1 = mad_sep(b[1], (double)r[1], bh);
            double x2 = mad_sep(b[2], (double)r[2], bw), y2 = mad_sep(b[3], (double)r[3], bh);
            square_box(x1, y1, x2, y2);
            o[0] = dfix(x1); o[1] = dfix(y1); o[2] = dfix(x2); o[3] = dfix(y2); o[4] = dfix((double)score);
            crop_row(o, img_w, img_h, tab_out + (size_t)k * 8);
        } else {
            o[0] = L.x1[i]; o[1] = L.y1[i]; o[2] = L.x2[i]; o[3] = L.y2[i]; o[4] = (double)score;
            const double* b = boxes_in + (size_t)src * 5;       // landmarks relative to the box BEFORE the regression
            const double bw = b[2] - b[0] + 1.0, bh = b[3] - b[1] + 1.0;
            const float* q = pts + (size_t)src * 10;
            float* po = points_out + (size_t)k * 10;
#pragma unroll
            for (int e = 0; e < 5; ++e) {
                po[e] = (float)__dadd_rn(__dadd_rn(__dmul_rn(bw, (double)q[e]), b[0]), -1.0);
                po[5 + e] = (float)__dadd_rn(__dadd_rn(__dmul_rn(bh, (double)q[5 + e]), b[1]), -1.0);
            }
        }
    }
    if (tid == 0) counters[STAGE] = nk;
}

}  // namespace

}  // namespace hsefr
