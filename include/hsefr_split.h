/*
 * hsefr_split.h -- C ABI of libhsefr_split.so: the same-photo split of every cluster of a face clustering, on the device in one pass
 * (hse_facerec_tf_amd/clustering.py, split_same_photo; the reference's age_gender_identity/facial_clustering.py:247-259: two faces of
 * one photo are two people).
 *
 * What it replaces in the reference, for ALL clusters of a clustering at once:
 *   - dist_matrix[np.ix_(cluster, cluster)] + inf_dist for two faces of one photo        facial_clustering.py:250-256
 *   - hac.linkage(squareform(.), 'complete') + hac.fcluster(., inf_dist / 2, 'distance')  facial_clustering.py:257-258
 *
 * A library of its own, as the five before it: libhsefr.so stays as it is (its size is bounded by its tests) and the seven share no
 * symbol -- this one has its own version number and its own per-thread error string.  Its clustering distance w(i,j) is the code of
 * libhsefr.so (csrc/linkage_scan.h: feat_tile), compiled twice with the same flags, so a cluster is split on the bits it was formed by.
 *
 * Conventions: those of hsefr.h, whose status values and hsefr_stream_t this header uses -- extern "C", plain C types, 0 on success or a
 * negative hsefr_status, never throws, data pointers are DEVICE pointers owned by the caller, launches are asynchronous on `stream`.
 * Built for gfx950 only.
 */
#ifndef HSEFR_SPLIT_H
#define HSEFR_SPLIT_H

#include "hsefr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSEFR_SPLIT_VERSION 100

/* the size classes of a group's chain: up to HSEFR_SPLIT_WAVE_MAX members one wave with the matrix in its 8 KiB of LDS, up to
 * HSEFR_SPLIT_LDS_MAX one workgroup with the matrix in LDS, above that one workgroup on the matrix in global memory */
#define HSEFR_SPLIT_WAVE_MAX 32
#define HSEFR_SPLIT_LDS_MAX 128

/* what `stats` counts */
#define HSEFR_SPLIT_STAT_EARLY 0   /* groups answered without a chain (one member, or no entry above cut)  */
#define HSEFR_SPLIT_STAT_LDS 1     /* groups whose chain ran in LDS (both LDS classes)                       */
#define HSEFR_SPLIT_STAT_GLOBAL 2  /* groups whose chain ran on the global slab                              */
#define HSEFR_SPLIT_STAT_MERGES 3  /* merges performed by those chains                                       */
#define HSEFR_SPLIT_STAT_BAD 4     /* members outside [0, n)                                                 */
#define HSEFR_SPLIT_STATS 5

int hsefr_split_version(void);

/* the last failure on the calling thread ("" before the first) */
const char* hsefr_split_last_error(void);

/*
 * Complete linkage inside every group of points, cut at `cut`, with `penalty` added between two points of one photo.
 *
 * The distance source is hsefr_hier_linkage's: exactly one of x [n,d] fp32 features (d a positive multiple of 8) with optional born / year
 * [n] (they come together), and dense [n,n] fp64, read as its upper triangle dense[min(i,j), max(i,j)] and never written.
 *   members        DEVICE int32 [offsets_host[groups]]: the points of group g are members[offsets_host[g] .. offsets_host[g + 1])
 *   offsets_host   HOST [groups + 1]: starts at 0, strictly increases, ends below 2^31; checked completely before any device work
 *   photo          DEVICE int32 [n]
 *   sublabel       DEVICE int32 [offsets_host[groups]]
 *   dist_out       DEVICE fp64, optional (may be NULL): the sum over the groups of k^2 values
 *   stats          DEVICE int64 [HSEFR_SPLIT_STATS], optional (may be NULL)
 * Group g of k members m_0 .. m_(k-1), in the order given, has the matrix P[a][b] = w(m_a, m_b) + penalty * [photo[m_a] == photo[m_b]]
 * (a != b), w the source's distance: feat_tile's value widened to fp64, or dense[min][max].  sublabel[offsets_host[g] + a] is
 * fcluster(linkage(squareform(P), 'complete'), cut, 'distance')[a] with the labels renumbered 0 .. c - 1 by first occurrence, found by the
 * nearest-neighbour chain with scipy's tie rules -- the chain starts at the lowest live slot; the previous chain element wins a tie,
 * otherwise the lowest index; the merged cluster is kept in the higher slot; the chain is kept across merges -- so equal P give equal
 * labels, ties included (clustering.complete_linkage_labels is the same procedure on the host).  A group with no entry above `cut` is one
 * cluster and runs no chain: complete linkage's heights are monotone and its last one is the largest entry.
 * dist_out receives every group's P as first built, row-major, group after group; its diagonal is unspecified.
 * A member outside [0, n) is never used as an address: its group gets sublabels -1, and stats counts every such member.
 * The workspace -- the sum of k^2 doubles plus O(members + groups) words -- is ONE stream-ordered allocation, refused (HSEFR_ERR_NOMEM,
 * with a message) before any launch.  The number of launches does not depend on `groups`: at most four kernels (one build, one chain
 * per size class that has a group) behind one copy of the group table and at most two memsets.  The library itself never synchronises.
 * The table goes up by hipMemcpyAsync from pageable host memory that is released when the call returns, as the tables of
 * hsefr_mixed.h do: that rests on the runtime finishing or staging a pageable source before it returns, and whether the runtime makes
 * the host wait for earlier work on `stream` while it does so has not been measured.
 * HSEFR_ERR_INVALID, before any device call, for n < 1, both or neither source, d not a positive multiple of 8, born without year (or the
 * reverse, or with dense), a null members, offsets_host, photo or sublabel, groups < 0, an offset table that does not start at 0, does not
 * strictly increase or reaches 2^31, a penalty that is not finite or is negative, and a cut that is not finite.  groups == 0 returns 0
 * and does nothing.
 */
int hsefr_split_groups(const float* x, int n, int d, const float* born, const float* year, const double* dense, const int* members,
                       const long long* offsets_host, int groups, const int* photo, double penalty, double cut, int* sublabel,
                       double* dist_out, long long* stats, hsefr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif
