/*
 * hsefr_shift.h -- C ABI of libhsefr_shift.so: mean-shift clustering of face features on the device, the scikit-learn branch's third
 * method in the clustering study (age_gender_identity/facial_clustering_test.py:210, :264: MeanShift(bandwidth=0.7).fit(all_features))
 * and the one clustering of the study that works from the features and not from a distance matrix
 * (hse_facerec_tf_amd/clustering.py: mean_shift, mean_shift_predict, cluster_faces_mean_shift, mean_shift_scores).
 *
 * What it replaces in the reference: sklearn.cluster.MeanShift(bandwidth=h, seeds=None, bin_seeding=False, max_iter=m).fit(X) and
 * .predict(Q), as scikit-learn 1.7.2 executes them (sklearn/cluster/_mean_shift.py; tests/mean_shift_ref.py restates it in NumPy), with
 * all seeds advanced together: every row of X is a seed, an iteration of all active seeds is two fp64 matrix products, and the only
 * N x N object is a BIT matrix (one bit per pair: 10.5 MB at 9164 faces).
 *
 * The ninth library of the package (hse_facerec_tf_amd/_lib.py: LIBRARIES; csrc/build.sh: LIBS): a library of its own as the seven
 * later ones before it -- libhsefr.so stays as it is, nothing is shared but the status values below, its own version and per-thread
 * error string.
 *
 * Conventions: those of hsefr.h, whose status values this header uses -- extern "C", plain C types, 0 on success or a negative
 * hsefr_status, never throws, data pointers are DEVICE pointers owned by the caller, `stream` is a hipStream_t.  Built for gfx950 only.
 */
#ifndef HSEFR_SHIFT_H
#define HSEFR_SHIFT_H

#include <stddef.h>
#include <stdint.h>

#include "hsefr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSEFR_SHIFT_VERSION 100

/* limits, refused beyond them with HSEFR_ERR_UNSUPPORTED */
#define HSEFR_SHIFT_MAX_N 65535          /* faces (and queries, and centres) */
#define HSEFR_SHIFT_MAX_D 4096           /* d is a multiple of HSEFR_SHIFT_D_MULTIPLE: 4 .. HSEFR_SHIFT_MAX_D */
#define HSEFR_SHIFT_D_MULTIPLE 4
#define HSEFR_SHIFT_MAX_ITER 10000       /* max_iter: 0 .. HSEFR_SHIFT_MAX_ITER */

/* the words of `info` (8 int32) */
enum {
    HSEFR_SHIFT_INFO_CENTERS = 0,        /* cluster centres: the rows of `centers` and of `intensity` that were written */
    HSEFR_SHIFT_INFO_N_ITER = 1,         /* scikit-learn's n_iter_: the largest number of completed iterations of a seed */
    HSEFR_SHIFT_INFO_DISTINCT = 2,       /* distinct means before the suppression */
    HSEFR_SHIFT_INFO_MAX_ITER = 3,       /* seeds stopped by max_iter and not by the shift test */
    HSEFR_SHIFT_INFO_NONFINITE = 4,      /* 1: a NaN or an infinity among the features; refused, nothing else was computed */
    HSEFR_SHIFT_INFO_INTERNAL = 5,       /* 1: an index left its bound on the device; it was not followed, and the call failed */
    HSEFR_SHIFT_INFO_WORK = 6,           /* seed-iterations done: the sum over the iterations of the seeds then active */
    HSEFR_SHIFT_INFO_WORDS = 8
};

/*
 * The arithmetic.  fp64 throughout: the fp32 features are widened in registers (exact); means, sums, distances and thresholds are doubles.
 *
 * Membership |x - m| <= h is decided as  D2 = fl(fl(N(m) + N(x)) - 2 P(m, x)) <= fl(h * h), where P is the fp64 MFMA product
 * (v_mfma_f64_16x16x4_f64: d fused multiply-adds into one accumulator) and N(v) = sum v_k^2 (fused multiply-adds over 64 interleaved
 * partial sums, then six additions).  With u = 2^-53:  |P - <m,x>| <= d u |m| |x|,  |N(v) - |v|^2| <= (d/64 + 7) u |v|^2 <= d u |v|^2 for
 * d >= 8 (and (d + 3) u in general), the two additions add 2 u of the whole, h * h carries u h^2, and three more u cover the terms of second order.  So
 *
 *     | D2 - |x - m|^2 |  +  | fl(h h) - h^2 |   <=   HSEFR_SHIFT_DIST2_ULPS(d) * 2^-53 * ((|m| + |x|)^2 + h^2)
 *
 * and, because | |x - m|^2 - h^2 | >= | |x - m| - h | h, the device's decision is the exact one for every pair with
 *
 *     | |x - m| - h |   >   HSEFR_SHIFT_DIST2_ULPS(d) * 2^-53 * ((|m| + |x|)^2 + h^2) / h .
 *
 * (ops.mean_shift_distance_bound states the right-hand side in Python; a mean of unit-norm rows has norm <= 1: 1.9e-13 at d = 256, h = 0.7.)
 * The same D2 decides which centres a centre suppresses and which centre is nearest to a face; label_dist, the shift |new - old| and
 * the centres' order are computed from differences and comparisons of the doubles themselves.
 *
 * A mean is  (sum over the member rows in index order) / count  on the same MFMA, the member bits expanded to 0.0 / 1.0 in registers:
 * one accumulator per element walks ALL n rows in one order whatever the seed (a chunk of 64 rows that none of a tile's seeds holds is
 * skipped: it would add zeros), with no split sum and no floating-point atomics.  Two seeds with equal member sets therefore reach
 * bit-identical means -- what the collapse of equal means relies on -- and two runs give identical bytes.
 */
#define HSEFR_SHIFT_DIST2_ULPS(d) ((d) + 8)

int hsefr_shift_version(void);

/* the last failure on the calling thread ("" before the first) */
const char* hsefr_shift_last_error(void);

/* bytes of workspace hsefr_shift_fit needs for n faces of d features (two n x d fp64 matrices, the n x ceil(n/64) bit matrix and O(n)
 * words); 0 for an n or d hsefr_shift_fit refuses */
size_t hsefr_shift_workspace_bytes(int n, int d);

/*
 * MeanShift(bandwidth, max_iter=max_iter).fit(x): x [n, d] fp32, never written.
 *   centers      fp64 [n, d]: the first info[0] rows are cluster_centers_, in scikit-learn's order ((count, coordinates) descending,
 *                a centre not yet suppressed suppressing every later one within the bandwidth); the other rows are not written
 *   intensity    int32 [n]: the first info[0] entries are the centres' member counts, the rest 0
 *   labels       int32 [n]: the index of the face's nearest centre, the lowest index among equal distances (cluster_all=True)
 *   label_dist   fp64 [n]: its distance to that centre (cluster_all=False is: label -1 where label_dist > bandwidth)
 *   info         int32 [8]: HSEFR_SHIFT_INFO_*
 *   workspace    at least hsefr_shift_workspace_bytes(n, d) bytes, 16-byte aligned (as centers; x: 8-byte aligned)
 * A seed stops when its mean moved by <= 1e-3 * bandwidth or when its completed iterations equal max_iter (so max_iter = 0 is one mean
 * update of every seed), and iterations launch over the seeds still active.  The call synchronises `stream` (it reads 64 bytes per
 * iteration: how many seeds go on) and returns with it drained; every loop on the host and the device is bounded by max_iter or n.
 *
 * HSEFR_ERR_INVALID before any device work: a null pointer, n < 1, a bandwidth that is not finite and > 0, a workspace that is too
 * small or misaligned.  HSEFR_ERR_UNSUPPORTED before any device work: n, d or max_iter beyond the limits above.
 * HSEFR_ERR_INVALID with info[4] = 1 for a non-finite feature; HSEFR_ERR_HIP with info[5] = 1 should an index leave its bound.
 */
int hsefr_shift_fit(const float* x, int n, int d, double bandwidth, int max_iter, double* centers, int32_t* intensity, int32_t* labels,
                    double* label_dist, int32_t* info, void* workspace, size_t workspace_bytes, void* stream);

/*
 * MeanShift.predict: for each of q's nq rows ([nq, d] fp32) the index of the nearest of `centers` ([k, d] fp64), the lowest index among
 * equal distances, and its distance (a non-finite row: -1 and NaN).  Asynchronous on `stream`; its nq + k doubles of workspace are one
 * stream-ordered allocation.  HSEFR_ERR_INVALID for a null pointer, nq < 1 or k < 1; HSEFR_ERR_UNSUPPORTED for nq, k or d beyond the limits.
 */
int hsefr_shift_assign(const float* q, int nq, int d, const double* centers, int k, int32_t* labels, double* dist, void* stream);

#ifdef __cplusplus
}
#endif

#endif
