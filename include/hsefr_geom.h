/*
 * hsefr_geom.h -- C ABI of libhsefr_geom.so: centroid, median and Ward linkage on the device, the three "geometric" methods of the
 * clustering study's list (age_gender_identity/facial_clustering_test.py:514) that hsefr_hier_linkage (hsefr.h) does not take
 * (hse_facerec_tf_amd/clustering.py: linkage_geometric, linkage_geometric_dense).
 *
 * What it replaces in the reference: hac.linkage(squareform(D), method) for method in 'centroid', 'median', 'ward'.
 *
 * A library of its own, as the six before it: libhsefr.so stays as it is (its size is bounded by its tests) and the eight share no
 * symbol -- this one has its own version number and its own per-thread error string.  Its working matrix and Ward's rounds are the code
 * of libhsefr.so (csrc/hier_linkage.hip over csrc/linkage_scan.h), compiled a second time with the same flags, so there is one
 * clustering distance in the project.
 *
 * Conventions: those of hsefr.h, whose status values and hsefr_stream_t this header uses -- extern "C", plain C types, 0 on success or a
 * negative hsefr_status, never throws, data pointers are DEVICE pointers owned by the caller, launches are asynchronous on `stream`.
 * Built for gfx950 only.
 */
#ifndef HSEFR_GEOM_H
#define HSEFR_GEOM_H

#include "hsefr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSEFR_GEOM_VERSION 100

enum { HSEFR_GEOM_CENTROID = 0, HSEFR_GEOM_MEDIAN = 1, HSEFR_GEOM_WARD = 2 };

/* centroid / median: up to HSEFR_GEOM_LDS_MAX points run as one launch of one workgroup with the matrix in LDS, more as two small
 * launches per merge on the matrix in global memory */
#define HSEFR_GEOM_LDS_MAX 128      /* largest n of the one-workgroup class */

int hsefr_geom_version(void);

/* the last failure on the calling thread ("" before the first) */
const char* hsefr_geom_last_error(void);

/*
 * The n - 1 merges of centroid, median or Ward linkage of n points.
 *
 * source: exactly one of x [n,d] fp32 (d a positive multiple of 8, optional born / year [n], which come together) and dense [n,n] fp64
 * read as its upper triangle dense[min(i,j), max(i,j)] and never written -- hsefr_hier_linkage's sources, checked the same way.
 *   merge_a, merge_b   int32 [n-1]: merge_a < merge_b, the slots (points) whose clusters merged
 *   merge_h            fp64 [n-1]: the height of the merge
 *   merge_round        int32 [n-1]: Ward: the round of the merge; centroid / median: the step index, which is the record's index
 *   w_out              optional (may be NULL) n*n doubles: the working matrix as first built (bitwise symmetric, diagonal +inf)
 *   counts             optional (may be NULL) device long long[2] = {records written, radicands clamped at zero}
 *
 * The update rules are scipy's _hierarchy_distance_update.pxi operation by operation in fp64, without contraction; x, y merge, i is the
 * third cluster, s their sizes:
 *   centroid  sqrt(max(((sx*dxi*dxi + sy*dyi*dyi) - (sx*sy*dxy*dxy)/(sx+sy)) / (sx+sy), 0))
 *   median    sqrt(max(0.5*(dxi*dxi + dyi*dyi) - 0.25*dxy*dxy, 0))
 *   ward      t = 1/(sx+sy+si);  sqrt(max((si+sx)*t*dxi*dxi + (si+sy)*t*dyi*dyi - si*t*dxy*dxy, 0))
 * The max(., 0) is this library's: it is scipy's value wherever that is a number, and 0 where rounding or a matrix that is not Euclidean
 * makes the radicand negative and scipy's sqrt gives NaN.  Every strictly negative radicand counts one in counts[1].
 *
 * HSEFR_GEOM_WARD runs hsefr_hier_linkage's rounds (every pair of mutually nearest clusters merges in the same round; two pairs merged in
 * one round update their common entry by scipy's two steps one after the other, the lower survivor's first): the cluster lives on in
 * merge_a's slot, records come round by round, and the call returns with `stream` synchronised (the host reads the cluster count once
 * per 32 rounds).  The tree is scipy's; the heights agree to rounding.
 * HSEFR_GEOM_CENTROID and _MEDIAN are not reducible -- their trees have inversions -- so the merges are sequential: n - 1 steps, each
 * merging the least pair under the total order (distance, lower slot, higher slot) and keeping the cluster in merge_b's slot, which is
 * scipy's tree and its heights bit for bit where the distances have no ties.  Records come in merge order; heights may fall.  The call
 * never synchronises: counts[0] == n - 1 confirms, after the stream has drained, that every step found a pair (a matrix of NaNs may not).
 *
 * The workspace -- the n x n fp64 working matrix plus O(n) words -- is ONE stream-ordered allocation, refused (HSEFR_ERR_NOMEM, with a
 * message) before any launch.  No grid-wide barriers, no cooperative launches, no persistent kernels.
 * HSEFR_ERR_INVALID, before any device call, for n < 1, both or neither source, d not a positive multiple of 8, born without year (or the
 * reverse, or with dense), a method that is none of the three, and a null merge_a, merge_b, merge_h or merge_round.  n == 1 writes no
 * record (counts = {0, 0}).
 */
int hsefr_geom_linkage(const float* x, int n, int d, const float* born, const float* year, const double* dense, int method,
                       int* merge_a, int* merge_b, double* merge_h, int* merge_round, double* w_out, long long* counts,
                       hsefr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
